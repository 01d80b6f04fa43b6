"""TEST INFRASTRUCTURE: CPU restatement of the REGULARISERS of the reference's ReconstructionLoss (models/bts/model/loss.py:192-245,
261-281) -- alpha_reg (ray | slice), surfaceness, ray entropy, depth_reg / depth_smoothness -- on top of the photometric term of
tests/_loss_pixel_oracle.py, for S scales with the fine dicts aliased to the coarse ones (trainer.py:247-248).  Pinned to the REAL
reference by tests/golden/loss_reg.npz (tests/golden/gen_golden_loss_reg.py) in tests/test_loss_reg_cpu.py.

``mutant`` swaps ONE of the reference's quirks for the plausible wrong reading; the golden's generator asserts that each of them moves
the loss, a logged term or a gradient beyond the GPU tests' bars on at least one configuration:
    last_in_sum        the last sample included in A
    cap_k_minus_1      cap = (K - 1) * fraction
    gate_strict        clamp_min's gradient with > instead of >=
    cap_unmasked       cap not multiplied by keep
    entropy_log2       log2 inside the entropy as well
    entropy_no_eps     the entropy without the 1e-5
    entropy_unmasked   the entropy not multiplied by keep
    entropy_scaled     the entropy divided by the number of scales
    surf_mask_always   surfaceness masked by the strict rule under policy none
    surf_mask_never    surfaceness not masked under an invalid policy
    sign0_is_1         d |x| / d x = 1 at x = 0
    depth_masked       the depth term multiplied by keep
    depth_borders      depth differences across the patch borders of a sample"""
import math
import os

import numpy as np
import torch

from tests import _loss_pixel_oracle as PO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_reg.npz")
# the smallest layouts at which each path of csrc/bts_loss_reg.hip can still go wrong
LAYOUTS = {
    "p8": dict(n=2, pc=3, h=8, w=8, K=8, nv=4, S=3),        # eight rays per wave; three scales
    "p2": dict(n=1, pc=5, h=2, w=2, K=64, nv=1, S=1),       # the smallest patch with both kinds of depth edges; one ray per wave
    "odd": dict(n=2, pc=1, h=17, w=23, K=48, nv=4, S=1),    # RE10K's K; B no multiple of anything; sample 1 more than half invalid
    "k130": dict(n=1, pc=1, h=5, w=7, K=130, nv=1, S=1),    # K > 64: a lane holds three samples, the last one ragged
}
ALL = dict(lambda_alpha_reg=0.05, lambda_surfaceness_reg=0.1, lambda_entropy=0.02, lambda_depth_reg=0.03, lambda_depth_smoothness=0.02)
CONFIGS = {
    "alpha_ray": dict(invalid_policy="weight_guided", lambda_alpha_reg=0.05, alpha_reg_reduction="ray"),
    "alpha_slice": dict(invalid_policy="weight_guided", lambda_alpha_reg=0.05, alpha_reg_reduction="slice"),
    "surf": dict(invalid_policy="weight_guided", lambda_surfaceness_reg=0.1),
    "entropy": dict(invalid_policy="weight_guided", lambda_entropy=0.02),
    "depth": dict(invalid_policy="weight_guided", lambda_depth_reg=0.03, lambda_depth_smoothness=0.02),
    "all_wg": dict(ALL, invalid_policy="weight_guided", alpha_reg_reduction="ray"),             # fed per-sample weights / invalid
    "all_strict_lean": dict(ALL, invalid_policy="strict", alpha_reg_reduction="slice"),         # fed invalid_wsum / invalid_any + alphas
    "all_none": dict(ALL, invalid_policy="none", alpha_reg_reduction="ray"),
    "diverse": dict(invalid_policy="weight_guided_diverse", native_pixel_loss=True, lambda_alpha_reg=0.05, lambda_surfaceness_reg=0.1,
                    lambda_depth_reg=0.03),
}
LEAN = ("all_strict_lean",)
DICT_KEYS = ["loss_rgb_coarse", "loss_rgb_fine", "loss_ray_entropy", "loss_depth_reg", "loss_alpha_reg", "loss_eas", "loss_depth_smoothness",
             "loss_invalid_ratio", "loss"]
TERM_KEYS = ["loss_ray_entropy", "loss_depth_reg", "loss_alpha_reg", "loss_depth_smoothness"]
MUTANTS = ("last_in_sum", "cap_k_minus_1", "gate_strict", "cap_unmasked", "entropy_log2", "entropy_no_eps", "entropy_unmasked",
           "entropy_scaled", "surf_mask_always", "surf_mask_never", "sign0_is_1", "depth_masked", "depth_borders")
# the constructed blocks of layout p8, scale 0: (sample, patch, rows)
TIE_BLOCK = (0, 1, slice(4, 6))       # A == cap exactly on 16 kept rays
CARRIED_ROW = (1, 2, 5)               # a slice row whose sum one ray carries over the cap


def config_of(name):
    return dict(CONFIGS[name], criterion="l1+ssim")


def rgb_samps_of(code, K, nv):
    """The per-sample colours of weight_guided_diverse from one byte per ray: code >= 200 is a ray without diversity (one colour for
    every sample of every view), below that the colours cycle through k / 4 with the sample index.  (n, pc, h, w) -> (.., K, nv, 3)"""
    c = code.to(torch.int64)[..., None, None, None]
    k = torch.arange(K).view(K, 1, 1)
    v = torch.arange(nv).view(1, nv, 1)
    ch = torch.arange(3).view(1, 1, 3)
    cyc = (k * (1 + c % 3) + v + 2 * ch + c) % 4
    return torch.where(c >= 200, (c % 4).expand(cyc.shape), cyc).float() / 4


def load_inputs(z, layout):
    """The golden's compact storage -> the float32 tensors the reference was fed (every step is exact in fp32): alphas as k / 256 with
    k in [0, 256], depth as k / 4096, colours as k / 256, weights as integer draws normalised per ray, the diverse colours from one
    byte per ray.  -> (levels: one dict per scale, scale 0 with the invalid-ray inputs; rgb_gt)"""
    L = LAYOUTS[layout]
    f = lambda k: torch.from_numpy(z[f"{layout}_{k}"].astype(np.float32))
    q = f("weights_u8")
    masks = dict(weights=q / q.sum(-1, keepdim=True), invalid=f("invalid"),
                 rgb_samps=rgb_samps_of(torch.from_numpy(z[f"{layout}_samp_code"]), L["K"], L["nv"]))
    alphas, depth, rgb = f("alphas_u16") / 256, f("depth_u16") / 4096, f("rgb_u8") / 256
    levels = [dict(masks, alphas=alphas[s], depth=depth[s], rgb=rgb[s]) for s in range(L["S"])]
    return levels, f("rgb_gt_u8") / 256


def lean_of(level):
    """the renderer's per-ray reductions that stand in for weights / invalid (lean training outputs), plus alphas"""
    w, i = level["weights"], level["invalid"]
    out = {k: v for k, v in level.items() if k not in ("weights", "invalid", "rgb_samps")}
    out.update(invalid_wsum=(i * w.unsqueeze(-1)).sum(-2), invalid_any=i.amax(-2))
    return out


def _abs(x, mutant):
    return x.abs() + (x == 0).to(x.dtype) * x if mutant == "sign0_is_1" else x.abs()       # same value; gradient 1 at 0


def _clamp_min0(x, mutant):
    return torch.where(x > 0, x, x * 0) if mutant == "gate_strict" else x.clamp_min(0)


def depth_term(d, mutant=None, keep=None):
    """mean((d[y+1] - d[y])^2) + mean((d[x+1] - d[x])^2) inside the patches; d (n, pc, h, w)"""
    if mutant == "depth_borders":
        n, pc, h, w = d.shape
        d = d.reshape(n, 1, pc * h, w)
    dy, dx = (d[:, :, 1:, :] - d[:, :, :-1, :]) ** 2, (d[:, :, :, 1:] - d[:, :, :, :-1]) ** 2
    if mutant == "depth_masked":
        dy, dx = dy * keep[:, :, :-1, :], dx * keep[:, :, :, :-1]
    return dy.mean() + dx.mean()


def regularisers(level, keep, config, scale, n_scales, mutant=None, keep_strict=None):
    """One scale's regulariser terms -> dict(alpha_reg, surf, entropy, depth) of 0-dim tensors (absent: the lambda is 0) and their share
    of the loss BEFORE the division by n_scales (the entropy's share is returned apart: it is added after)."""
    ignore = config.get("invalid_policy", "strict") not in (None, "none")
    out, loss, after = {}, 0.0, 0.0
    if config.get("lambda_depth_reg", 0) > 0 or config.get("lambda_depth_smoothness", 0) > 0:
        s = depth_term(level["depth"], mutant, keep)
        out["depth"] = s
        loss = loss + s * (config.get("lambda_depth_reg", 0) + config.get("lambda_depth_smoothness", 0))
    if config.get("lambda_alpha_reg", 0) > 0:
        a = level["alphas"]
        K = a.shape[-1]
        a_sum = (a if mutant == "last_in_sum" else a[..., :-1]).sum(-1)
        cap = torch.ones_like(a_sum) * ((K - 1 if mutant == "cap_k_minus_1" else K) * config.get("alpha_reg_fraction", 1 / 8))
        if ignore:
            a_sum, cap = a_sum * keep, (cap if mutant == "cap_unmasked" else cap * keep)
        if config.get("alpha_reg_reduction", "ray") == "ray":
            s = _clamp_min0(a_sum - cap, mutant)
        else:
            s = _clamp_min0(a_sum.sum(dim=-1) - cap.sum(dim=-1), mutant) / a_sum.shape[-1]
        s = s.mean()
        out["alpha_reg"] = s
        loss = loss + s * config["lambda_alpha_reg"]
    if config.get("lambda_surfaceness_reg", 0) > 0:
        a = level["alphas"]
        p = (-torch.log(torch.exp(-_abs(a, mutant)) + torch.exp(-_abs(1 - a, mutant)))).mean(-1)
        if (ignore and mutant != "surf_mask_never"):
            p = p * keep
        elif not ignore and mutant == "surf_mask_always":
            p = p * keep_strict
        s = p.mean()
        out["surf"] = s
        loss = loss + s * config["lambda_surfaceness_reg"]
    if scale == 0 and config.get("lambda_entropy", 0) > 0:
        a = level["alphas"] + (0.0 if mutant == "entropy_no_eps" else 1e-5)
        dens = a / a.sum(dim=-1, keepdim=True)
        logd = torch.log2(dens) if mutant == "entropy_log2" else torch.log(dens)
        if mutant == "entropy_no_eps":
            logd = torch.where(dens > 0, logd, torch.zeros_like(logd))          # (0 log 0 = 0 instead of NaN)
        ent = -(dens * logd).sum(-1) / math.log2(a.shape[-1])
        if mutant != "entropy_unmasked":
            ent = ent * keep
        s = ent.mean()
        out["entropy"] = s
        after = s * config["lambda_entropy"] / (n_scales if mutant == "entropy_scaled" else 1)
    return out, loss, after


def reconstruction_loss(levels, rgb_gt, config, mutant=None):
    """-> (loss, dict in the reference's keys, dict(keep (n, pc, h, w), surf: the never-logged surfaceness term summed over the scales))"""
    S = len(levels)
    level0 = levels[0]
    policy = config.get("invalid_policy", "strict")
    invalid = PO.invalid_rays(level0, policy if policy not in (None, "none") else "none")
    keep = 1 - invalid.squeeze(-1).to(level0["alphas"].dtype)
    keep_strict = 1 - PO.invalid_rays(level0, "strict").squeeze(-1).to(level0["alphas"].dtype)
    loss, after = 0.0, 0.0
    d = dict.fromkeys(DICT_KEYS, 0.0)
    surf = 0.0
    for s, level in enumerate(levels):
        lv = dict(level0, rgb=level["rgb"], depth=level["depth"])
        photo, o = PO.reconstruction_loss(lv, rgb_gt, dict(config, lambda_edge_aware_smoothness=0))
        loss = loss + photo
        d["loss_rgb_coarse"] += o["loss_rgb"].item() * config.get("lambda_coarse", 1)
        d["loss_rgb_fine"] += o["loss_rgb"].item() * config.get("lambda_fine", 1)
        terms, share, aft = regularisers(level, keep, config, s, S, mutant, keep_strict)
        loss, after = loss + share, after + aft
        if "depth" in terms and config.get("lambda_depth_reg", 0) > 0:
            d["loss_depth_reg"] += terms["depth"].item()
        if "depth" in terms and config.get("lambda_depth_smoothness", 0) > 0:
            d["loss_depth_smoothness"] += terms["depth"].item()
        if "alpha_reg" in terms:
            d["loss_alpha_reg"] += terms["alpha_reg"].item()
        if "entropy" in terms:
            d["loss_ray_entropy"] = terms["entropy"].item()
        if "surf" in terms:
            surf = surf + terms["surf"].item()
    loss = loss / S + after
    d["loss_invalid_ratio"] = invalid.float().mean().item()
    d["loss"] = loss.item()
    return loss, d, dict(keep=keep, surf=surf)


def leaves(levels, dtype=torch.float32):
    """levels with alphas and depth of every scale as fresh leaves of `dtype` -> (levels, [alphas_0, depth_0, alphas_1, ...])"""
    out, lv = [], []
    for level in levels:
        level = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in level.items()}
        level["alphas"], level["depth"] = level["alphas"].clone().requires_grad_(True), level["depth"].clone().requires_grad_(True)
        out.append(level)
        lv += [level["alphas"], level["depth"]]
    return out, lv


def grads(loss, lv):
    """d loss / d every leaf, zeros where the loss does not depend on it"""
    g = torch.autograd.grad(loss, lv, allow_unused=True)
    return [torch.zeros_like(x) if y is None else y for x, y in zip(lv, g)]
