"""GPU: the opt-in `native_pixel_loss: true` of ReconstructionLoss -- criterion l1 / l2 with or without median thresholding under the four
invalid-ray policies (bts_pixel_loss, csrc/bts_loss_pixel.hip) and l1+ssim under weight_guided_diverse (bts_loss_diverse_flags + the
shipped loss kernels) -- against tests/golden/loss_pixel.npz (the REAL reference's ReconstructionLoss on four layouts and six
configurations) and the CPU restatement tests/_loss_pixel_oracle.py (pinned to that golden in tests/test_loss_pixel_cpu.py).  The bars
of tests/test_gpu_loss.py / test_gpu_loss_frames.py: loss within 1e-5, invalid ratio 1e-6, smoothness term 1e-5 relative, gradients
within 1e-4 of the largest entry; the per-sample thresholds are torch.equal to the reference's (e is one subtraction, one abs or multiply
and a min: bit-exact) and the kept count is equal as an integer.  The golden's generator asserts that no (ray, view) is within 1e-4 of a
comparison of the diverse rule, so no ray is set aside anywhere.

The smoothness cross-check against bts_photometric_loss_tiled has no bar fixed in advance: the tiled kernel's own distance to an fp64
evaluation on the same inputs is measured in the test and the new entry may differ from the tiled kernel by 4 x that.  Measured on
MI355X over the four layouts (sum: relative, the tiled kernel's per-patch terms added exactly and rounded to fp32 once; g_depth: of the
largest entry): the tiled kernel is 9.1e-10 .. 6.4e-8 (sum) and 8.3e-8 .. 1.4e-7 (g_depth) from fp64; the new entry is 0.0 from the tiled
kernel in both -- its smoothness passes keep that kernel's tile geometry and order of sums, so the test also asserts torch.equal."""
import numpy as np
import pytest
import torch

from tests import _loss_pixel_oracle as PO

pytestmark = pytest.mark.gpu
KEY = {"native_pixel_loss": True}
_CACHE = {}


def _golden(layout):
    """the layout's inputs (CPU tensors), loaded once and left unchanged"""
    if "z" not in _CACHE:
        _CACHE["z"] = np.load(PO.GOLDEN)
    if layout not in _CACHE:
        _CACHE[layout] = PO.load_inputs(_CACHE["z"], layout)
    return _CACHE["z"], _CACHE[layout][0], _CACHE[layout][1]


def _hip(level_cpu, gt, config, lean=None, grad=True):
    """ReconstructionLoss on the GPU -> loss, dict, d rgb, d depth.  lean: the (B, nv) invalid_wsum / invalid_any dict that replaces the
    per-sample tensors"""
    import behindthescenes_amd as bts
    r1, d1 = level_cpu["rgb"].detach().cuda().requires_grad_(grad), level_cpu["depth"].detach().cuda().requires_grad_(grad)
    level = {k: v.cuda() for k, v in (lean if lean is not None else level_cpu).items() if k not in ("rgb", "depth")}
    level.update(rgb=r1, depth=d1)
    crit = bts.ReconstructionLoss(dict(config, **KEY))
    loss, parts = crit(dict(coarse=[level], fine=[dict(level)], rgb_gt=gt.cuda()))
    if grad:
        loss.backward()
    return loss, parts, r1.grad, d1.grad


def _flat(level, gt):
    """the flat device tensors of native.pixel_loss / photometric_loss"""
    n, pc, h, w, nv, _ = level["rgb"].shape
    K = level["weights"].shape[-1]
    f = lambda t, *tail: t.reshape((-1,) + tail).float().contiguous().cuda()
    return dict(rgb=f(level["rgb"], nv * 3), depth=f(level["depth"]), weights=f(level["weights"], K), invalid=f(level["invalid"], K, nv),
                rgb_samps=f(level["rgb_samps"], K, nv, 3), rgb_gt=f(gt, 3)), (n, h, w)


def _native(level, gt, cname, need_grad=True, **over):
    from behindthescenes_amd import native
    t, (n, h, w) = _flat(level, gt)
    c = PO.CONFIGS[cname]
    kw = dict(invalid_wsum=None, invalid_any=None)
    kw.update(over)
    return native.pixel_loss(t["rgb"], t["depth"], t["weights"], t["invalid"], t["rgb_gt"], n, h, w, c.get("criterion", "l2"),
                             c.get("invalid_policy", "strict"), c.get("median_thresholding", False), True, 1.0, 1.0, need_grad=need_grad,
                             rgb_samps=t["rgb_samps"], **kw)


def _check(loss, parts, g_r, g_d, ref, ref_parts, ref_gr, ref_gd, tag):
    print(tag, "loss", loss.item(), ref, "eas", parts["loss_eas"], ref_parts["loss_eas"], "invalid", parts["loss_invalid_ratio"],
          ref_parts["loss_invalid_ratio"])
    errs = {}
    for got, want, name in ((g_r.cpu(), ref_gr, "rgb"), (g_d.cpu(), ref_gd, "depth")):
        errs[name] = (got - want).abs().max().item() / want.abs().max().clamp_min(1e-20).item()
    print(tag, "gradient errors", errs)
    assert abs(loss.item() - ref) <= 1e-5, (loss.item(), ref)
    assert abs(parts["loss_invalid_ratio"] - ref_parts["loss_invalid_ratio"]) <= 1e-6
    assert abs(parts["loss_eas"] - ref_parts["loss_eas"]) <= 1e-5 * max(1.0, abs(ref_parts["loss_eas"]))
    for k in ("loss_rgb_coarse", "loss_rgb_fine"):
        assert abs(parts[k] - ref_parts[k]) <= 1e-5, k
    for name, err in errs.items():
        assert err <= 1e-4, (name, err)


@pytest.mark.parametrize("cname", list(PO.CONFIGS))
@pytest.mark.parametrize("layout", list(PO.LAYOUTS))
def test_loss_vs_the_real_reference(layout, cname):
    z, level, gt = _golden(layout)
    key = f"{layout}_{cname}"
    want = dict(zip(PO.DICT_KEYS, z[f"{key}_loss_dict"].tolist()))
    got = _hip(level, gt, PO.config_of(cname))
    assert list(got[1]) == ["loss_rgb_coarse", "loss_rgb_fine", "loss_ray_entropy", "loss_depth_reg", "loss_alpha_reg", "loss_eas",
                            "loss_depth_smoothness", "loss_invalid_ratio", "loss"]
    _check(*got, z[f"{key}_loss"].item(), want, torch.from_numpy(z[f"{key}_g_rgb"]), torch.from_numpy(z[f"{key}_g_depth"]), key)


@pytest.mark.parametrize("cname", ["l1_median", "l2_median"])
@pytest.mark.parametrize("layout", list(PO.LAYOUTS))
def test_thresholds_and_kept_count_equal_the_references(layout, cname):
    z, level, gt = _golden(layout)
    key = f"{layout}_{cname}"
    out, thr, kept, g_rgb, g_depth = _native(level, gt, cname)
    print(key, "thresholds", thr.tolist(), z[f"{key}_thresholds"].tolist(), "kept", kept.item(), int(z[f"{key}_kept"][0]))
    assert torch.equal(thr.cpu(), torch.from_numpy(z[f"{key}_thresholds"]))
    assert kept.item() == int(z[f"{key}_kept"][0]) == int(out[3].item())
    assert (thr[-1].item() == 0.0) == (layout == "odd")


@pytest.mark.parametrize("cname", ["l1", "l2_diverse"])
def test_without_median_the_count_is_every_value(cname):
    z, level, gt = _golden("odd")
    out, thr, kept, _, _ = _native(level, gt, cname)
    assert thr is None and kept is None and int(out[3].item()) == 3 * level["depth"].numel()


def test_two_scales_and_unequal_lambdas_vs_the_restatement():
    """the per-scale loop: its own thresholds per scale, the smoothness term divided by 2 ** scale, lambda_coarse / lambda_fine on the
    aliased fine dict, scale 0's invalid-ray inputs for every scale"""
    import behindthescenes_amd as bts
    _, level, gt = _golden("p8")
    g = torch.Generator().manual_seed(5)
    level1 = dict(level, rgb=(level["rgb"] + 0.05 * torch.randn(level["rgb"].shape, generator=g)), depth=level["depth"] * 1.5 + 0.25)
    cfg = dict(PO.config_of("l2_median"), lambda_coarse=0.7, lambda_fine=0.4)
    leaves, ref = [], 0.0
    for s, lv in enumerate((level, level1)):
        lv = dict(lv, rgb=lv["rgb"].clone().requires_grad_(True), depth=lv["depth"].clone().requires_grad_(True))
        lv.update(weights=level["weights"], invalid=level["invalid"])
        _, o = PO.reconstruction_loss(lv, gt, cfg)
        ref = ref + o["loss_rgb"] * (0.7 + 0.4) + o["loss_eas"] * PO.LAMBDA_EAS / 2 ** s
        leaves += [lv["rgb"], lv["depth"]]
    ref = ref / 2
    ref_g = torch.autograd.grad(ref, leaves)
    dev = [{k: v.cuda() for k, v in lv.items()} for lv in (level, level1)]
    for lv in dev:
        lv["rgb"].requires_grad_(True), lv["depth"].requires_grad_(True)
    crit = bts.ReconstructionLoss(dict(cfg, **KEY))
    loss, parts = crit(dict(coarse=dev, fine=[dict(lv) for lv in dev], rgb_gt=gt.cuda()))
    loss.backward()
    print("two scales", loss.item(), ref.item())
    assert abs(loss.item() - ref.item()) <= 1e-5 and abs(parts["loss"] - ref.item()) <= 1e-5
    for got, want in zip([dev[0]["rgb"].grad, dev[0]["depth"].grad, dev[1]["rgb"].grad, dev[1]["depth"].grad], ref_g):
        assert (got.cpu() - want).abs().max().item() <= 1e-4 * want.abs().max().item()


@pytest.mark.parametrize("layout", list(PO.LAYOUTS))
def test_ssim_with_diverse_equals_strict_fed_host_formed_flags(layout):
    """HIP against HIP: l1+ssim + weight_guided_diverse is bts_loss_diverse_flags + the shipped kernels under the strict policy"""
    from behindthescenes_amd import native
    _, level, gt = _golden(layout)
    wsum, std = PO.diverse_stats(level)
    flags = ((wsum > .9) | (std < 0.01)).float()                     # formed on the host
    t, _ = _flat(level, gt)
    dev_flags = native.loss_diverse_flags(t["rgb_samps"], t["weights"], t["invalid"])
    assert torch.equal(dev_flags.cpu(), flags.reshape(-1, flags.shape[-1])) and 0 < flags.mean() < 1
    a = _hip(level, gt, dict(criterion="l1+ssim", invalid_policy="weight_guided_diverse", lambda_edge_aware_smoothness=PO.LAMBDA_EAS))
    b = _hip(level, gt, dict(criterion="l1+ssim", invalid_policy="strict", lambda_edge_aware_smoothness=PO.LAMBDA_EAS),
             lean=dict(invalid_any=flags, invalid_wsum=torch.zeros_like(flags)))
    assert torch.equal(a[0], b[0]) and dict(a[1]) == dict(b[1])
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and a[1]["loss_invalid_ratio"] > 0


def test_one_sample_per_ray_makes_the_std_nan_and_the_flag_false():
    """K == 1: torch's unbiased std is NaN, NaN < .01 is false -- only the weight rule can flag"""
    from behindthescenes_amd import native
    g = torch.Generator().manual_seed(3)
    B, nv = 300, 2
    samps, w = torch.rand(B, 1, nv, 3, generator=g), torch.rand(B, 1, generator=g) * 0.2 + 0.85
    w[(w - 0.9).abs() < 1e-3] = 0.95
    inv = (torch.rand(B, 1, nv, generator=g) < 0.5).float()
    got = native.loss_diverse_flags(samps.cuda(), w.cuda(), inv.cuda()).cpu()
    assert torch.equal(got, ((inv * w.unsqueeze(-1)).sum(-2) > .9).float()) and 0 < got.mean() < 1


@pytest.mark.parametrize("layout", list(PO.LAYOUTS))
def test_smoothness_matches_the_tiled_kernel(layout):
    """HIP against HIP: out[1] and g_depth of bts_pixel_loss against bts_photometric_loss_tiled on the same depth, ground truth and keep
    flags (strict, from the same `invalid`); the margin is 4 x the tiled kernel's own distance to an fp64 evaluation (module docstring)"""
    import ctypes as C
    from behindthescenes_amd import _lib, native
    _, level, gt = _golden(layout)
    t, (n, h, w) = _flat(level, gt)
    B, nv, K = t["rgb_gt"].shape[0], level["rgb"].shape[-2], level["weights"].shape[-1]
    parts = torch.empty(B // (h * w), 4, device="cuda")
    tg_rgb, tg_depth = torch.empty_like(t["rgb"]), torch.empty_like(t["depth"])
    a = _lib.BtsLossArgs(rgb=t["rgb"].data_ptr(), depth=t["depth"].data_ptr(), weights=None, invalid=t["invalid"].data_ptr(),
                         rgb_gt=t["rgb_gt"].data_ptr(), parts=parts.data_ptr(), g_rgb=tg_rgb.data_ptr(), g_depth=tg_depth.data_ptr(),
                         n_patches=B // (h * w), patch_h=h, patch_w=w, nv=nv, K=K, invalid_policy=1, edge_aware_smoothness=1, scale_rgb=1.0,
                         scale_eas=1.0, invalid_wsum=None, invalid_any=None)
    native.photometric_loss_tiled(a, parts, tg_rgb, tg_depth, native._stream(t["rgb"]))
    out, _, _, _, g_depth = _native(level, gt, "l2")
    keep = 1 - PO.invalid_rays(level, "strict").squeeze(-1).float()
    s64, g64 = PO.eas_fp64(gt, level["depth"], keep)
    tiled_sum = parts[:, 1].double().sum().float().item()          # the tiled kernel's per-patch terms, added exactly and rounded to fp32 once
    d_sum = abs(tiled_sum - s64.item()) / abs(s64.item())
    d_g = (tg_depth.cpu().double() - g64.reshape(-1)).abs().max().item() / g64.abs().max().item()
    e_sum = abs(out[1].item() - tiled_sum) / abs(s64.item())
    e_g = (g_depth - tg_depth).abs().max().item() / g64.abs().max().item()
    print(layout, "tiled vs fp64: sum", d_sum, "g_depth", d_g, "| pixel vs tiled: sum", e_sum, "g_depth", e_g, "| g_depth bit-identical",
          torch.equal(g_depth, tg_depth))
    assert int(out[2].item()) == int(parts[:, 2].sum().item()) > 0
    assert e_sum <= 4 * d_sum, (e_sum, d_sum)
    assert e_g <= 4 * d_g, (e_g, d_g)
    assert torch.equal(g_depth, tg_depth) and out[1].item() == tiled_sum       # the same geometry, the same order of sums: the same bits


@pytest.mark.parametrize("cname", ["l1_median", "l2_median"])
def test_lean_inputs_give_identical_results(cname):
    """invalid_any (strict) / invalid_wsum (weight_guided) in place of weights / invalid: identical keep flags, identical everything"""
    _, level, gt = _golden("odd")
    w, i = level["weights"], level["invalid"]
    lean = dict(invalid_wsum=(i * w.unsqueeze(-1)).sum(-2), invalid_any=i.amax(-2))
    full, ln = _hip(level, gt, PO.config_of(cname)), _hip(level, gt, PO.config_of(cname), lean=lean)
    assert torch.equal(full[0], ln[0]) and dict(full[1]) == dict(ln[1])
    assert torch.equal(full[2], ln[2]) and torch.equal(full[3], ln[3])
    assert full[1]["loss_invalid_ratio"] > 0
    nv = level["rgb"].shape[-2]
    a = _native(level, gt, cname)
    b = _native(level, gt, cname, invalid_wsum=lean["invalid_wsum"].reshape(-1, nv).contiguous().cuda(),
                invalid_any=lean["invalid_any"].reshape(-1, nv).contiguous().cuda())
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("cname", ["l2", "l1_median", "l2_diverse"])
def test_no_grad_runs_the_forward_only_and_gives_the_same_value(cname):
    _, level, gt = _golden("odd")
    with torch.no_grad():
        l0, p0, _, _ = _hip(level, gt, PO.config_of(cname), grad=False)
    l1, p1, g_r, g_d = _hip(level, gt, PO.config_of(cname))
    assert not l0.requires_grad and l1.requires_grad and g_r is not None and g_d is not None
    assert torch.equal(l0, l1.detach()) and dict(p0) == dict(p1)
    out, thr, kept, g_rgb, g_depth = _native(level, gt, cname, need_grad=False)
    assert g_rgb is None and g_depth is None and torch.isfinite(out).all()


@pytest.mark.parametrize("cname", ["l2", "l1_median", "l2_median", "l2_diverse"])
def test_reruns_are_bit_identical(cname):
    _, level, gt = _golden("frame")
    a, b = _native(level, gt, cname), _native(level, gt, cname)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)
    assert a[3].abs().max() > 0 and a[4].abs().max() > 0


def test_the_fused_training_step_runs_an_opted_in_l2_criterion_entry_by_entry():
    import behindthescenes_amd as bts
    from behindthescenes_amd import synthetic as S
    from behindthescenes_amd.train_step import FusedTrainStep
    n, V, H, W = 2, 4, 48, 160
    scene = S.synthetic_scene(n, V, H, W, 64, seed=5, baseline=0.4, smooth=True)
    torch.manual_seed(4)
    net = bts.BTSNet(S.field_conf(64, 64, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), 64, num_views=n)
    S.init_mlp_(net.mlp_coarse, seed=7)
    net = net.to("cuda").train()
    renderer = bts.NeRFRenderer.from_conf(dict(n_coarse=64, lindisp=True, hard_alpha_cap=True, lean_training_outputs=True)).to("cuda").train()
    sampler = bts.PatchRaySampler(ray_batch_size=512, z_near=3.0, z_far=80.0, patch_size=8)
    crit = bts.ReconstructionLoss(dict(criterion="l2", invalid_policy="strict", **KEY))
    step = FusedTrainStep(renderer.bind_parallel(net).train(), sampler, crit)
    torch.manual_seed(3)
    loss, loss_dict, data = step(*[scene[k].cuda() for k in ("images", "projs", "poses")], ids_encoder=[0], ids_render=[2, 3], ids_loss=[0, 1])
    assert step.last_path.startswith("entries:") and "criterion l2" in step.last_path
    # the criterion restated in torch on the entry-by-entry render (scales averaged; fine aliases coarse: lambda_coarse + lambda_fine = 2)
    c0 = data["coarse"][0]
    keep = 1 - torch.all(c0["invalid_any"] > .5, dim=-1, keepdim=True).float()
    want = sum(2 * (((c["rgb"] - data["rgb_gt"].unsqueeze(-2)) ** 2).amin(-2) * keep).mean() for c in data["coarse"]) / len(data["coarse"])
    print("fused step", loss.item(), want.item(), step.last_path)
    assert abs(loss.item() - want.item()) <= 1e-5 and abs(loss_dict["loss"] - want.item()) <= 1e-5
    loss.backward()
    grads = [p.grad for p in net.mlp_coarse.parameters()]
    assert grads and all(g is not None and torch.isfinite(g).all().item() for g in grads) and any(g.abs().max().item() > 0 for g in grads)
