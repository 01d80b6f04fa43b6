"""GPU: the opt-in `native_ssim_median: true` of ReconstructionLoss -- criterion l1+ssim WITH median_thresholding on
bts_photometric_loss_median (the median variant of csrc/bts_loss_tiled.hip's passes joined to the radix selection) -- against
tests/golden/loss_ssim_median.npz (the REAL reference's ReconstructionLoss on four layouts and five configurations) and the CPU
restatement tests/_loss_ssim_median_oracle.py (pinned to that golden, mutants included, in tests/test_loss_ssim_median_cpu.py).  The
project's bars for l1+ssim: loss within 1e-5, invalid ratio 1e-6, smoothness term 1e-5 relative, gradients within 1e-4 of the largest
entry.  The kept count equals the reference's as an integer: the golden's generator asserts that nothing lies within 20 D above any
threshold (D = the layout's largest distance of the fp32 reference's e from its own fp64 evaluation, 3.7e-6 .. 7.4e-6), so no rounding
difference between a kernel and the reference moves a pixel across a threshold.

The thresholds have no bar fixed in advance: each may be 2 D(layout) from the reference's threshold evaluated in fp64.  MEASURED on
MI355X, largest over the configurations, layouts p8 / ragged / odd / frame: the HIP thresholds are 2.5e-6 / 4.5e-6 / 4.0e-6 / 2.1e-6 from
the fp64 ones (bars 2 D = 7.5e-6 / 1.43e-5 / 1.26e-5 / 1.47e-5), the fp32 reference's 1.6e-6 / 2.4e-6 / 1.2e-6 / 3.3e-6 (the test prints
both distances for every layout and configuration).

The smoothness part is bts_photometric_loss_tiled's, bit for bit: columns 1 and 2 of `parts`, g_depth, and out[1] as the fp32 number
nearest to the sum of column 1.  Column 0 of `parts` (the sum of e BEFORE thresholding) on 8 x 8 patches is checked against the wave kernel
(native.photometric_loss) to 1e-6 of each entry, the bar of tests/test_gpu_loss_frames.py's cross-check of the two kernels."""
import numpy as np
import pytest
import torch

from tests import _loss_ssim_median_oracle as MO

pytestmark = pytest.mark.gpu
_CACHE = {}


def _golden(layout):
    """the layout's inputs (CPU tensors), loaded once and left unchanged"""
    if "z" not in _CACHE:
        _CACHE["z"] = np.load(MO.GOLDEN)
    if layout not in _CACHE:
        _CACHE[layout] = MO.load_inputs(_CACHE["z"], layout)
    return (_CACHE["z"],) + _CACHE[layout]


def _keys(cname):
    k = {"native_ssim_median": True}
    if cname == "diverse":
        k["native_pixel_loss"] = True
    if MO.automasked(cname):
        k["native_automask"] = True
    return k


def _device_level(level, cname, grad=True, rgb=None, depth=None):
    """the render dict on the GPU; "strict_lean": the (B, nv) reductions in place of the per-sample tensors"""
    r1 = (level["rgb"] if rgb is None else rgb).detach().cuda().requires_grad_(grad)
    d1 = (level["depth"] if depth is None else depth).detach().cuda().requires_grad_(grad)
    if cname == "strict_lean":
        w, i = level["weights"], level["invalid"]
        rest = dict(invalid_wsum=(i * w.unsqueeze(-1)).sum(-2).cuda(), invalid_any=i.amax(-2).cuda())
    else:
        rest = {k: v.cuda() for k, v in level.items() if k not in ("rgb", "depth")}
    return dict(rest, rgb=r1, depth=d1)


def _gt_in(gt, bound, cname):
    return (torch.cat((gt, bound.unsqueeze(-1)), dim=-1) if MO.automasked(cname) else gt).cuda()


def _hip(level, gt, bound, cname, grad=True, **over):
    """ReconstructionLoss on the GPU -> loss, dict, d rgb, d depth"""
    import behindthescenes_amd as bts
    dev = _device_level(level, cname, grad)
    crit = bts.ReconstructionLoss(dict(MO.config_of(cname), **_keys(cname), **over), use_automasking=MO.automasked(cname))
    loss, parts = crit(dict(coarse=[dev], fine=[dict(dev)], rgb_gt=_gt_in(gt, bound, cname)))
    if grad:
        loss.backward()
    return loss, parts, dev["rgb"].grad, dev["depth"].grad


def _flat(level, gt, bound):
    n, pc, h, w, nv, _ = level["rgb"].shape
    K = level["weights"].shape[-1]
    f = lambda t, *tail: t.reshape((-1,) + tail).float().contiguous().cuda()
    return dict(rgb=f(level["rgb"], nv * 3), depth=f(level["depth"]), weights=f(level["weights"], K), invalid=f(level["invalid"], K, nv),
                rgb_samps=f(level["rgb_samps"], K, nv, 3), rgb_gt=f(gt, 3), bound=f(bound)), (n, h, w, nv, K)


def _native(layout, cname, need_grad=True, parts=None):
    """native.photometric_loss_median on a layout under a configuration -> (out, thresholds, kept, g_rgb, g_depth), the flat tensors"""
    from behindthescenes_amd import native
    _, level, gt, bound = _golden(layout)
    t, (n, h, w, nv, K) = _flat(level, gt, bound)
    policy, kw = MO.CONFIGS[cname]["invalid_policy"], {}
    if cname == "diverse":
        policy, kw = "strict", dict(invalid_any=native.loss_diverse_flags(t["rgb_samps"], t["weights"], t["invalid"]))
    elif cname == "strict_lean":
        kw = dict(invalid_any=t["invalid"].amax(1).contiguous())
    res = native.photometric_loss_median(t["rgb"], t["depth"], t["weights"], t["invalid"], t["rgb_gt"], n, h, w, policy, True, 1.0, 1.0,
                                         need_grad=need_grad, thresh=t["bound"] if MO.automasked(cname) else None, parts=parts, **kw)
    return res, t


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


@pytest.mark.parametrize("cname", list(MO.CONFIGS))
@pytest.mark.parametrize("layout", list(MO.LAYOUTS))
def test_loss_vs_the_real_reference(layout, cname):
    z, level, gt, bound = _golden(layout)
    key = f"{layout}_{cname}"
    want = dict(zip(MO.DICT_KEYS, z[f"{key}_loss_dict"].tolist()))
    got = _hip(level, gt, bound, cname)
    assert list(got[1]) == ["loss_rgb_coarse", "loss_rgb_fine", "loss_ray_entropy", "loss_depth_reg", "loss_alpha_reg", "loss_eas",
                            "loss_depth_smoothness", "loss_invalid_ratio", "loss"]
    _check(*got, z[f"{key}_loss"].item(), want, torch.from_numpy(z[f"{key}_g_rgb"]), torch.from_numpy(z[f"{key}_g_depth"]), key)


@pytest.mark.parametrize("cname", list(MO.CONFIGS))
@pytest.mark.parametrize("layout", list(MO.LAYOUTS))
def test_kept_count_equals_the_references_and_thresholds_sit_within_2_d_of_fp64(layout, cname):
    z = _golden(layout)[0]
    key = f"{layout}_{cname}"
    n, pc, h, w, _, _ = MO.LAYOUTS[layout]
    (out, thr, kept, _, _), _ = _native(layout, cname)
    D = z[f"{layout}_D"].item()
    thr64, thr32 = torch.from_numpy(z[f"{key}_thresholds64"]), torch.from_numpy(z[f"{key}_thresholds"])
    d_hip, d_ref = (thr.cpu().double() - thr64).abs().max().item(), (thr32.double() - thr64).abs().max().item()
    print(key, "kept", kept.item(), int(z[f"{key}_kept"][0]), "| thresholds", thr.tolist(), "| distance to the fp64 thresholds: HIP", d_hip,
          "fp32 reference", d_ref, "| D", D)
    assert kept.item() == int(z[f"{key}_kept"][0]) == int(out[3].item())
    if layout == "p8":          # sample 0 keeps rank + 2 (the <= tie), sample 1 rank + 1
        assert kept.item() == 2 * ((pc * h * w - 1) // 2) + 3
    assert d_hip <= 2 * D, (d_hip, D)
    assert (thr[-1].item() == 0.0) == (layout == "odd" and cname != "none")


@pytest.mark.parametrize("cname", ["wg", "strict_lean", "wg_automask"])
@pytest.mark.parametrize("layout", list(MO.LAYOUTS))
def test_smoothness_is_the_tiled_kernels_bit_for_bit(layout, cname):
    """HIP against HIP: columns 1 and 2 of parts, out[1], out[2] and g_depth against bts_photometric_loss_tiled on the same inputs"""
    from behindthescenes_amd import _lib, native
    n, pc, h, w, nv, K = MO.LAYOUTS[layout]
    parts = torch.empty(n * pc, 4, device="cuda")
    (out, _, _, _, g_depth), t = _native(layout, cname, parts=parts)
    policy = {"wg": 2, "strict_lean": 1, "wg_automask": 2}[cname]
    t_parts = torch.empty_like(parts)
    tg_rgb, tg_depth = torch.empty_like(t["rgb"]), torch.empty_like(t["depth"])
    a = _lib.BtsLossArgs(rgb=t["rgb"].data_ptr(), depth=t["depth"].data_ptr(), weights=t["weights"].data_ptr(), invalid=t["invalid"].data_ptr(),
                         rgb_gt=t["rgb_gt"].data_ptr(), parts=t_parts.data_ptr(), g_rgb=tg_rgb.data_ptr(), g_depth=tg_depth.data_ptr(),
                         n_patches=n * pc, patch_h=h, patch_w=w, nv=nv, K=K, invalid_policy=policy, edge_aware_smoothness=1, scale_rgb=1.0,
                         scale_eas=1.0, invalid_wsum=None, invalid_any=None)
    native.photometric_loss_tiled(a, t_parts, tg_rgb, tg_depth, native._stream(t["rgb"]), t["bound"] if MO.automasked(cname) else None)
    assert torch.equal(parts[:, 1:], t_parts[:, 1:]) and t_parts[:, 1].abs().sum() > 0 and parts[:, 2].sum() > 0
    assert torch.equal(parts[:, 0], t_parts[:, 0])                       # (and the sum of e before thresholding: the same pass 1 arithmetic)
    assert out[1].item() == t_parts[:, 1].double().sum().float().item() and out[2].item() == t_parts[:, 2].sum().item()
    assert torch.equal(g_depth, tg_depth) and g_depth.abs().max() > 0


@pytest.mark.parametrize("cname", ["wg", "none", "wg_automask"])
def test_8x8_patches_before_thresholding_match_the_wave_kernel(cname):
    """a threshold of +inf cannot be asked for; column 0 of `parts` is the sum of e BEFORE thresholding: against the wave kernel's per-patch sums"""
    from behindthescenes_amd import native
    n, pc, h, w, nv, K = MO.LAYOUTS["p8"]
    parts = torch.empty(n * pc, 4, device="cuda")
    _, t = _native("p8", cname, need_grad=False, parts=parts)
    wave, _, _ = native.photometric_loss(t["rgb"], t["depth"], t["weights"], t["invalid"], t["rgb_gt"], h, w, MO.CONFIGS[cname]["invalid_policy"], True,
                                         1.0, 1.0, need_grad=False, thresh=t["bound"] if MO.automasked(cname) else None)
    rel = ((wave[:, 0] - parts[:, 0]).abs() / wave[:, 0].abs().clamp_min(1e-20)).max().item()
    print("p8", cname, "column 0 against the wave kernel: relative", rel, "absolute", (wave[:, 0] - parts[:, 0]).abs().max().item())
    assert h * w <= native.WAVE_PATCH_PIXELS and wave[:, 0].min() > 0
    assert (wave[:, 0] - parts[:, 0]).abs().max().item() <= 1e-6 and rel <= 1e-6
    assert torch.equal(wave[:, 2], parts[:, 2])


def _second_scale(level, gt):
    """another set of renders with the same two populations: the errors shrunk towards the ground truth"""
    return gt.unsqueeze(-2) + 0.75 * (level["rgb"] - gt.unsqueeze(-2)), level["depth"] * 1.5 + 0.25


def _gaps_hold(o, D):
    e, thr = o["e"].reshape(o["e"].shape[0], -1), o["thresholds"]
    return all((e[s][e[s] > thr[s]].min() - thr[s]).item() >= 20 * D for s in range(e.shape[0]))


def test_two_scales_and_unequal_lambdas_vs_the_restatement():
    """the per-scale loop: its own thresholds per scale, the smoothness term divided by 2 ** scale, lambda_coarse / lambda_fine on the
    aliased fine dict, scale 0's invalid-ray inputs for every scale"""
    import behindthescenes_amd as bts
    z, level, gt, _ = _golden("ragged")
    rgb1, depth1 = _second_scale(level, gt)
    cfg = dict(MO.config_of("wg"), lambda_coarse=0.7, lambda_fine=0.4)
    leaves, ref, thrs = [], 0.0, []
    for s, (r, d) in enumerate(((level["rgb"], level["depth"]), (rgb1, depth1))):
        lv = dict(level, rgb=r.clone().requires_grad_(True), depth=d.clone().requires_grad_(True))
        _, o = MO.reconstruction_loss(lv, gt, cfg)
        assert _gaps_hold(o, z["ragged_D"].item())          # (on the restatement: what makes the comparison meaningful at this scale too)
        ref = ref + o["loss_rgb"] * (0.7 + 0.4) + o["loss_eas"] * MO.LAMBDA_EAS / 2 ** s
        leaves += [lv["rgb"], lv["depth"]]
        thrs.append(o["thresholds"])
    assert not torch.equal(thrs[0], thrs[1])
    ref = ref / 2
    ref_g = torch.autograd.grad(ref, leaves)
    dev = [_device_level(level, "wg"), _device_level(level, "wg", rgb=rgb1, depth=depth1)]
    crit = bts.ReconstructionLoss(dict(cfg, **_keys("wg")))
    loss, parts = crit(dict(coarse=dev, fine=[dict(lv) for lv in dev], rgb_gt=gt.cuda()))
    loss.backward()
    print("two scales", loss.item(), ref.item())
    assert abs(loss.item() - ref.item()) <= 1e-5 and abs(parts["loss"] - ref.item()) <= 1e-5
    for got, want in zip([dev[0]["rgb"].grad, dev[0]["depth"].grad, dev[1]["rgb"].grad, dev[1]["depth"].grad], ref_g):
        assert (got.cpu() - want).abs().max().item() <= 1e-4 * want.abs().max().item()


def test_a_fine_dict_that_is_no_alias_makes_a_second_call(monkeypatch):
    import behindthescenes_amd as bts
    from behindthescenes_amd import native
    z, level, gt, _ = _golden("odd")
    rgb1, _ = _second_scale(level, gt)
    cfg = dict(MO.config_of("wg"), lambda_coarse=0.7, lambda_fine=0.4)
    calls, real = [], native.photometric_loss_median
    monkeypatch.setattr(native, "photometric_loss_median", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    crit = bts.ReconstructionLoss(dict(cfg, **_keys("wg")))
    coarse = _device_level(level, "wg")
    crit(dict(coarse=[coarse], fine=[dict(coarse)], rgb_gt=gt.cuda()))
    assert len(calls) == 1                                   # the aliased fine dict is served by the coarse launch
    del calls[:]
    fine = _device_level(level, "wg", rgb=rgb1)
    loss, parts = crit(dict(coarse=[coarse], fine=[fine], rgb_gt=gt.cuda()))
    assert len(calls) == 2
    loss.backward()
    lc = dict(level, rgb=level["rgb"].clone().requires_grad_(True), depth=level["depth"].clone().requires_grad_(True))
    lf = dict(level, rgb=rgb1.clone().requires_grad_(True))
    _, oc = MO.reconstruction_loss(lc, gt, cfg)
    _, of = MO.reconstruction_loss(lf, gt, dict(cfg, lambda_edge_aware_smoothness=0))
    assert _gaps_hold(oc, z["odd_D"].item()) and _gaps_hold(of, z["odd_D"].item())
    ref = oc["loss_rgb"] * 0.7 + of["loss_rgb"] * 0.4 + oc["loss_eas"] * MO.LAMBDA_EAS
    ref_g = torch.autograd.grad(ref, [lc["rgb"], lc["depth"], lf["rgb"]])
    print("separate fine dict", loss.item(), ref.item())
    assert abs(loss.item() - ref.item()) <= 1e-5
    assert abs(parts["loss_rgb_coarse"] - 0.7 * oc["loss_rgb"].item()) <= 1e-5 and abs(parts["loss_rgb_fine"] - 0.4 * of["loss_rgb"].item()) <= 1e-5
    for got, want in zip([coarse["rgb"].grad, coarse["depth"].grad, fine["rgb"].grad], ref_g):
        assert (got.cpu() - want).abs().max().item() <= 1e-4 * want.abs().max().item()
    assert fine["depth"].grad is None


@pytest.mark.parametrize("layout,cname", [("frame", "wg"), ("ragged", "wg_automask"), ("p8", "diverse")])
def test_reruns_are_bit_identical(layout, cname):
    (a, _), (b, _) = _native(layout, cname), _native(layout, cname)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[3].abs().max() > 0 and a[4].abs().max() > 0


def test_no_grad_runs_the_forward_only_and_gives_the_same_value():
    _, level, gt, bound = _golden("odd")
    with torch.no_grad():
        l0, p0, _, _ = _hip(level, gt, bound, "wg", grad=False)
    l1, p1, g_r, g_d = _hip(level, gt, bound, "wg")
    assert not l0.requires_grad and l1.requires_grad and g_r is not None and g_d is not None
    assert torch.equal(l0, l1.detach()) and dict(p0) == dict(p1)
    (out, thr, kept, g_rgb, g_depth), _ = _native("odd", "wg", need_grad=False)
    assert g_rgb is None and g_depth is None and torch.isfinite(out).all()
