"""GPU: the photometric loss on patches of more than 64 pixels and on whole frames (bts_photometric_loss_tiled, 16 x 16 tiles of a patch,
through the drop-in ReconstructionLoss) against the CPU oracle restatement of the reference's loss (oracle/bts_loss.py, pinned to the
real reference at these sizes by tests/golden/loss_frames.npz): value within 1e-5, invalid ratio 1e-6, smoothness term 1e-5 relative,
gradients with respect to rgb and depth within 1e-4 of the largest entry (the bars of tests/test_gpu_loss.py).

The shapes: just over the wave kernel's 64 pixels; exactly one tile; one more than a tile on both axes (remainder tiles 1 high and 7
wide); a small frame with interior tiles; one row; one column; one render view.  At every one of them the fp32 oracle is within 7e-6
(gradients) and 1e-7 (loss) of an fp64 evaluation and no pixel has its two smallest e_v closer than 1e-6, so no pixel is excluded."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import bts_loss as OL

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_frames.npz")
CONFIG = {"criterion": "l1+ssim", "lambda_edge_aware_smoothness": 0.01}


def _inputs(n, pc, h, w, nv, K, seed):
    """tests/test_gpu_loss.py::_inputs with two changes that the one-patch shapes need.  The band of fully invalid rays is a column band
    when h == 1 (a one-row patch would otherwise have loss and gradients all zero).  The original makes view 0 of patch 0 an exact match
    of the ground truth; with pc == 1 that is every pixel of the only patch, the rgb term is then zero and d loss / d rgb nothing but
    rounding noise of 1e-9 (the SSIM gradient at x == y is a difference of equal terms), against which no relative bar means anything
    -- so with pc == 1 the exact match covers the upper-left block of the patch and the rest stays noisy, and the depth below the
    clamp range sits in the only patch."""
    g = torch.Generator().manual_seed(seed)
    gt = F.avg_pool2d(torch.rand(n * pc, 3, h + 4, w + 4, generator=g), 3, 1, 1)[:, :, 2:-2, 2:-2]          # correlated like real frames
    gt = gt.reshape(n, pc, 3, h, w).permute(0, 1, 3, 4, 2).contiguous()
    rgb = (gt.unsqueeze(-2) + 0.15 * torch.randn(n, pc, h, w, nv, 3, generator=g)).clamp(0, 1)
    if pc > 1:
        rgb[:, 0, :, :, 0] = gt[:, 0]                              # an exact match: SSIM term 0, L1 gradient sign(0) = 0
    else:                                                          # ... on a block of the only patch (see the docstring)
        rgb[:, 0, : (h + 1) // 2, : (w + 1) // 2, 0] = gt[:, 0, : (h + 1) // 2, : (w + 1) // 2]
    depth = torch.rand(n, pc, h, w, generator=g) * 100 + 0.5       # beyond the [1e-3, 80] clamp on purpose
    depth[:, min(1, pc - 1), 0, 0] = 1e-4
    wts = torch.rand(n, pc, h, w, K, generator=g)
    wts = wts / wts.sum(-1, keepdim=True)
    inv = (torch.rand(n, pc, h, w, K, nv, generator=g) < 0.3).float()
    if h == 1:
        inv[:, :, :, 0, :, :] = 1.0                                 # a column of rays invalid in every view
        inv[:, :, :, 1, : K // 2, 0] = 0.0                          # ... and one valid in view 0 only
    else:
        inv[:, :, 0, :, :, :] = 1.0                                 # a row of rays invalid in every view
        inv[:, :, 1, :, : K // 2, 0] = 0.0                          # ... and one valid in view 0 only
    alphas = torch.rand(n, pc, h, w, K, generator=g)
    return rgb, depth, wts, inv, alphas, gt


_ORACLE = {}


def _oracle(shape, policy, dtype=torch.float32):
    """inputs and the CPU oracle's (loss, parts, d rgb, d depth) of one case, computed once"""
    key = (shape, policy, dtype)
    if key not in _ORACLE:
        n, pc, h, w, nv, K = shape
        rgb, depth, wts, inv, alphas, gt = _inputs(n, pc, h, w, nv, K, seed=h * 100 + nv)
        r0, d0 = rgb.clone().to(dtype).requires_grad_(True), depth.clone().to(dtype).requires_grad_(True)      # (leaves of their own)
        ref, ref_parts = OL.reconstruction_loss(dict(rgb=r0, depth=d0, weights=wts.to(dtype), invalid=inv.to(dtype), alphas=alphas.to(dtype)),
                                                gt.to(dtype), invalid_policy=policy, lambda_eas=0.01)
        g_r, g_d = torch.autograd.grad(ref, [r0, d0])
        _ORACLE[key] = ((rgb, depth, wts, inv, alphas, gt), ref.item(), {k: v.item() for k, v in ref_parts.items()}, g_r, g_d)
    return _ORACLE[key]


def _hip(level_cpu, gt, policy, lean=False):
    """ReconstructionLoss on the GPU -> loss, parts, d rgb, d depth"""
    import behindthescenes_amd as bts
    r1, d1 = level_cpu["rgb"].detach().cuda().requires_grad_(True), level_cpu["depth"].detach().cuda().requires_grad_(True)
    level = {k: v.cuda() for k, v in level_cpu.items() if k not in ("rgb", "depth")}
    if lean:      # the renderer's per-ray reductions, formed on the host from the per-sample tensors
        w, i = level_cpu["weights"], level_cpu["invalid"]
        level = dict(invalid_wsum=(i * w.unsqueeze(-1)).sum(-2).cuda(), invalid_any=i.amax(-2).cuda())
    level.update(rgb=r1, depth=d1)
    crit = bts.ReconstructionLoss(dict(CONFIG, invalid_policy=policy))
    loss, parts = crit(dict(coarse=[level], fine=[dict(level)], rgb_gt=gt.cuda()))
    loss.backward()
    return loss, parts, r1.grad, d1.grad


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
    for name, err in errs.items():
        assert err <= 1e-4, (name, err)


ALL = ["weight_guided", "strict", "none"]
CASES = [((1, 2, 9, 8, 2, 5), ["weight_guided"]), ((2, 3, 16, 16, 3, 5), ["weight_guided"]), ((1, 2, 17, 23, 2, 5), ALL),
         ((1, 2, 40, 72, 3, 5), ALL), ((1, 1, 1, 70, 2, 4), ["weight_guided"]), ((1, 1, 70, 1, 2, 4), ["weight_guided"]),
         ((1, 1, 33, 33, 1, 3), ["weight_guided"])]


@pytest.mark.parametrize("shape,policy", [(s, p) for s, ps in CASES for p in ps], ids=lambda v: "x".join(map(str, v[2:4])) if isinstance(v, tuple) else v)
def test_tiled_loss_vs_oracle(shape, policy):
    (rgb, depth, wts, inv, alphas, gt), ref, ref_parts, ref_gr, ref_gd = _oracle(shape, policy)
    got = _hip(dict(rgb=rgb, depth=depth, weights=wts, invalid=inv, alphas=alphas), gt, policy)
    _check(*got, ref, ref_parts, ref_gr, ref_gd, f"{shape} {policy}")


@pytest.mark.parametrize("policy", ["weight_guided", "strict"])
def test_lean_inputs_give_the_same_loss_and_gradients(policy):
    """invalid_wsum / invalid_any in place of weights / invalid: the keep flags are identical, so is everything else"""
    (rgb, depth, wts, inv, alphas, gt), *_ = _oracle((1, 2, 17, 23, 2, 5), policy)
    level = dict(rgb=rgb, depth=depth, weights=wts, invalid=inv)
    full, lean = _hip(level, gt, policy), _hip(level, gt, policy, lean=True)
    assert torch.equal(full[0], lean[0]) and dict(full[1]) == dict(lean[1])
    assert torch.equal(full[2], lean[2]) and torch.equal(full[3], lean[3])
    assert full[1]["loss_invalid_ratio"] > 0


@pytest.mark.parametrize("name", ["patch16", "frame"])
def test_tiled_loss_vs_the_real_reference(name):
    z = np.load(GOLDEN)
    t = {k: torch.from_numpy(z[f"{name}_{k}"]) for k in ("rgb", "depth", "weights", "invalid", "rgb_gt", "loss", "loss_dict", "g_rgb", "g_depth")}
    want = dict(zip(["loss_rgb_coarse", "loss_rgb_fine", "loss_eas", "loss_invalid_ratio", "loss"], t["loss_dict"].tolist()))
    got = _hip(dict(rgb=t["rgb"], depth=t["depth"], weights=t["weights"], invalid=t["invalid"].float()), t["rgb_gt"], "weight_guided")
    _check(*got, t["loss"].item(), want, t["g_rgb"], t["g_depth"], name)


def _native_args(rgb, depth, wts, inv, gt, ph, pw, policy=2):
    """flat device tensors and a filled BtsLossArgs for native-level calls"""
    from behindthescenes_amd import _lib
    nv, K = rgb.shape[-2], wts.shape[-1]
    t = dict(rgb=rgb.reshape(-1, nv * 3), depth=depth.reshape(-1), weights=wts.reshape(-1, K), invalid=inv.reshape(-1, K, nv), rgb_gt=gt.reshape(-1, 3))
    t = {k: v.float().contiguous().cuda() for k, v in t.items()}
    B = t["rgb_gt"].shape[0]
    t["parts"] = torch.empty(B // (ph * pw), 4, device="cuda")
    t["g_rgb"], t["g_depth"] = torch.empty_like(t["rgb"]), torch.empty_like(t["depth"])
    a = _lib.BtsLossArgs(n_patches=B // (ph * pw), patch_h=ph, patch_w=pw, nv=nv, K=K, invalid_policy=policy, edge_aware_smoothness=1,
                         scale_rgb=0.37, scale_eas=0.011, invalid_wsum=None, invalid_any=None, **{k: v.data_ptr() for k, v in t.items()})
    return a, t


def test_tiled_kernel_equals_the_wave_kernel_on_8x8_patches():
    import ctypes as C
    from behindthescenes_amd import _lib, native
    rgb, depth, wts, inv, alphas, gt = _inputs(2, 5, 8, 8, 3, 5, seed=803)
    outs = []
    for tiled in (False, True):
        a, t = _native_args(rgb, depth, wts, inv, gt, 8, 8)
        stream = native._stream(t["rgb"])
        if tiled:
            native.photometric_loss_tiled(a, t["parts"], t["g_rgb"], t["g_depth"], stream)
        else:
            _lib.check(_lib.load().bts_photometric_loss(C.byref(a), stream), "bts_photometric_loss")
        outs.append({k: t[k].cpu() for k in ("parts", "g_rgb", "g_depth")})
    wave, tile = outs
    assert wave["parts"].shape == (10, 4) and wave["parts"][:, 2].sum() > 0
    assert torch.equal(wave["parts"][:, 2:], tile["parts"][:, 2:])                     # invalid counts
    rel = ((wave["parts"][:, :2] - tile["parts"][:, :2]).abs() / wave["parts"][:, :2].abs().clamp_min(1e-20)).max().item()
    print("parts", rel)
    assert rel <= 1e-6
    for k in ("g_rgb", "g_depth"):
        err = (wave[k] - tile[k]).abs().max().item() / wave[k].abs().max().item()
        print(k, err)
        assert err <= 1e-6, (k, err)


def test_reruns_are_bit_identical():
    from behindthescenes_amd import native
    (rgb, depth, wts, inv, alphas, gt), *_ = _oracle((1, 2, 40, 72, 3, 5), "weight_guided")
    outs = []
    for _ in range(2):
        a, t = _native_args(rgb, depth, wts, inv, gt, 40, 72)
        native.photometric_loss_tiled(a, t["parts"], t["g_rgb"], t["g_depth"], native._stream(t["rgb"]))
        outs.append(t)
    for k in ("parts", "g_rgb", "g_depth"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert outs[0]["g_rgb"].abs().max() > 0 and outs[0]["g_depth"].abs().max() > 0


def test_no_grad_value_equals_the_grad_mode_value():
    import behindthescenes_amd as bts
    (rgb, depth, wts, inv, alphas, gt), *_ = _oracle((1, 2, 40, 72, 3, 5), "weight_guided")
    crit = bts.ReconstructionLoss(dict(CONFIG, invalid_policy="weight_guided"))
    level = dict(rgb=rgb.cuda(), depth=depth.cuda(), weights=wts.cuda(), invalid=inv.cuda())
    with torch.no_grad():
        l0, p0 = crit(dict(coarse=[level], fine=[dict(level)], rgb_gt=gt.cuda()))
    level = dict(level, rgb=rgb.cuda().requires_grad_(True), depth=depth.cuda().requires_grad_(True))
    l1, p1 = crit(dict(coarse=[level], fine=[dict(level)], rgb_gt=gt.cuda()))
    assert not l0.requires_grad and l1.requires_grad
    assert torch.equal(l0, l1.detach()) and dict(p0) == dict(p1)


def test_one_validation_frame():
    """the size loss_during_validation calls the criterion with: ImageRaySampler.reconstruct's (n, v, H, W, nv, 3) at 192 x 640.

    The oracle is evaluated in fp64 here.  Unlike at the shapes above, its fp32 evaluation is NOT within 7e-6 of the fp64 one at this
    size: among 245 760 pixels one (frame 1, row 31, column 539, blue) has the SSIM clamp's argument 1 - n / d = 0.99999956 in fp64 and
    1.0000021 in torch's fp32 (cancellation in the variances: 2.6e-6 of rounding), so the fp32 oracle cuts that pixel's SSIM gradient
    off and differs from its own fp64 evaluation by 1.66e-2 of the largest entry around it (measured on the CPU alone).  The HIP
    kernel's fp32 falls on the fp64 side: against the fp32 oracle it shows the same 1.66e-2 at that pixel."""
    shape = (1, 2, 192, 640, 1, 8)
    (rgb, depth, wts, inv, alphas, gt), ref, ref_parts, ref_gr, ref_gd = _oracle(shape, "weight_guided", torch.float64)
    ref_gr, ref_gd = ref_gr.float(), ref_gd.float()
    got = _hip(dict(rgb=rgb, depth=depth, weights=wts, invalid=inv, alphas=alphas), gt, "weight_guided")
    _check(*got, ref, ref_parts, ref_gr, ref_gd, "192x640")


def _net(H, W, n, train):
    import behindthescenes_amd as bts
    from behindthescenes_amd import synthetic as S
    torch.manual_seed(4)
    net = bts.BTSNet(S.field_conf(64, 64, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), 64, num_views=n)
    S.init_mlp_(net.mlp_coarse, seed=7)
    net = net.to("cuda")
    return net.train() if train else net.eval()


def test_frame_rendered_by_the_hip_renderer_end_to_end():
    """encode -> ImageRaySampler.sample -> HIP renderer (want_weights, want_alphas) -> reconstruct -> ReconstructionLoss on a 24 x 40 frame
    with v = 2, against the oracle on the CPU copy of the same render dict"""
    import behindthescenes_amd as bts
    from behindthescenes_amd import synthetic as S
    H, W = 24, 40
    scene = S.synthetic_scene(1, 2, H, W, 64, seed=9, intrinsics=S.K_KITTIRAW, smooth=True)
    net = _net(H, W, 1, train=False)
    wrapped = bts.NeRFRenderer.from_conf(dict(n_coarse=16, lindisp=True, hard_alpha_cap=True)).bind_parallel(net).eval().to("cuda")
    frame = bts.FusedEvalFrame(wrapped, bts.ImageRaySampler(3.0, 80.0), fused=False)
    torch.manual_seed(21)
    data = frame(*[scene[k].cuda() for k in ("images", "projs", "poses")], ids_encoder=[0], ids_render=[0, 1], want_weights=True, want_alphas=True,
                 to_z=False)
    assert frame.last_path.startswith("entries")
    c = data["coarse"][0]
    assert c["rgb"].shape == (1, 2, H, W, 2, 3) and c["weights"].shape == (1, 2, H, W, 16)
    crit = bts.ReconstructionLoss(dict(CONFIG, invalid_policy="weight_guided"))
    grads, losses = [], []
    for dev in ("cuda", "cpu"):
        level = {k: v.detach().to(dev) for k, v in c.items()}
        level["rgb"].requires_grad_(True), level["depth"].requires_grad_(True)
        gt = data["rgb_gt"].detach().to(dev)
        if dev == "cuda":
            loss, _ = crit(dict(coarse=[level], fine=[dict(level)], rgb_gt=gt))
        else:
            loss, _ = OL.reconstruction_loss(level, gt, invalid_policy="weight_guided", lambda_eas=0.01)
        grads.append([g.cpu() for g in torch.autograd.grad(loss, [level["rgb"], level["depth"]])])
        losses.append(loss.item())
    print("loss", losses)
    assert abs(losses[0] - losses[1]) <= 1e-5
    for got, want, name in zip(grads[0], grads[1], ("rgb", "depth")):
        err = (got - want).abs().max().item() / want.abs().max().clamp_min(1e-20).item()
        print(name, err)
        assert err <= 1e-4, (name, err)


def test_a_training_step_with_the_trainers_default_patch():
    """PatchRaySampler(patch_size=16): FusedTrainStep answers "patches of more than 64 pixels", runs entry by entry -- and the criterion
    at the end of that sequence now completes"""
    import behindthescenes_amd as bts
    from behindthescenes_amd import synthetic as S
    from behindthescenes_amd.train_step import FusedTrainStep
    n, V, H, W = 2, 4, 48, 160
    scene = S.synthetic_scene(n, V, H, W, 64, seed=5, baseline=0.4, smooth=True)
    net = _net(H, W, n, train=True)
    renderer = bts.NeRFRenderer.from_conf(dict(n_coarse=64, lindisp=True, hard_alpha_cap=True, lean_training_outputs=True)).to("cuda").train()
    sampler = bts.PatchRaySampler(ray_batch_size=512, z_near=3.0, z_far=80.0, patch_size=16)
    crit = bts.ReconstructionLoss(dict(CONFIG, invalid_policy="weight_guided"))
    step = FusedTrainStep(renderer.bind_parallel(net).train(), sampler, crit)
    torch.manual_seed(3)
    loss, loss_dict, data = step(*[scene[k].cuda() for k in ("images", "projs", "poses")], ids_encoder=[0], ids_render=[2, 3], ids_loss=[0, 1])
    assert step.last_path.startswith("entries") and "64 pixels" in step.last_path
    assert data["coarse"][0]["rgb"].shape[2:4] == (16, 16)
    loss.backward()
    assert torch.isfinite(loss).item() and loss.item() > 0
    grads = [p.grad for p in net.mlp_coarse.parameters()]
    assert grads and all(g is not None and torch.isfinite(g).all().item() for g in grads) and any(g.abs().max().item() > 0 for g in grads)
