"""TEST INFRASTRUCTURE: CPU restatement of the reference's ReconstructionLoss (models/bts/model/loss.py:139-167) for criterion l1+ssim WITH
median_thresholding -- what the opt-in `native_ssim_median: true` opens -- with or without the automasking bound, for one scale with the
fine dict aliased to the coarse one.  Pinned to the REAL reference by tests/golden/loss_ssim_median.npz
(tests/golden/gen_golden_loss_ssim_median.py) in tests/test_loss_ssim_median_cpu.py.  Works in the inputs' dtype: fed doubles it is the
fp64 yardstick of the thresholds.

``mutant`` swaps ONE of the reference's quirks for the plausible wrong reading; the golden's generator asserts that each of them moves the
stored loss, kept count or a gradient beyond the tests' bars on at least one layout:
    upper_median      rank N / 2 instead of torch.median's lower (N - 1) / 2
    strict_less       e < thr instead of e <= thr
    mask_at_receiver  the kept flag applied to the pixel that RECEIVES the gradient instead of the pixel whose error it is (under SSIM a
                      kept pixel's error reaches its 3 x 3 neighbours' colours whether or not those neighbours are kept)
    rank_before_keep  the median taken before the invalid-ray mask (invalid rays then do not rank as zeros)
    rank_before_bound the median taken before the automasking bound"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import bts_loss as OL
from tests import _loss_pixel_oracle as PO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_ssim_median.npz")
LAYOUTS = {"p8": (2, 4, 8, 8, 3, 4), "ragged": (2, 2, 20, 36, 2, 4), "odd": (3, 1, 17, 23, 2, 5), "frame": (1, 1, 40, 72, 1, 4)}   # (n, pc, h, w, nv, K)
LAMBDA_EAS = 0.01
CONFIGS = {
    "wg": dict(invalid_policy="weight_guided"),
    "strict_lean": dict(invalid_policy="strict"),                 # the HIP side gets invalid_any instead of invalid
    "none": dict(invalid_policy="none"),
    "diverse": dict(invalid_policy="weight_guided_diverse"),
    "wg_automask": dict(invalid_policy="weight_guided"),          # with the seeded bound map as rgb_gt's fourth channel
}
DICT_KEYS = PO.DICT_KEYS
MUTANTS = ("upper_median", "strict_less", "mask_at_receiver", "rank_before_keep", "rank_before_bound")


def config_of(name):
    return dict(CONFIGS[name], criterion="l1+ssim", median_thresholding=True, lambda_edge_aware_smoothness=LAMBDA_EAS)


def automasked(name):
    return name.endswith("_automask")


def load_inputs(z, layout):
    """-> (level, rgb_gt (n, pc, h, w, 3), bound (n, pc, h, w)) from the golden's compact exact storage (_loss_pixel_oracle.load_inputs)"""
    level, gt = PO.load_inputs(z, layout)
    return level, gt, torch.from_numpy(z[f"{layout}_bound"])


def errors(level, rgb_gt):
    """loss.py:151-153 -> (e (n, pc, h, w, 1) = the minimum over the views, all views' e_v (n, pc, h, w, nv))"""
    ev = OL.errors_l1ssim(level["rgb"], rgb_gt.unsqueeze(-2))
    return ev.amin(-2), ev.squeeze(-1)


def reconstruction_loss(level, rgb_gt, config, bound=None, mutant=None):
    """-> (loss, dict(loss_rgb, loss_eas, loss_invalid_ratio, thresholds (n), kept, keep (n, pc, h, w), e (n, pc, h, w) as ranked))"""
    policy = config.get("invalid_policy", "strict")
    ignore = policy not in (None, "none")
    lam_eas = config.get("lambda_edge_aware_smoothness", 0)
    dt = level["rgb"].dtype
    b = level["rgb"].shape[0]
    invalid = PO.invalid_rays(level, policy if ignore else "none")
    keep = 1 - invalid.to(dt)
    e0, _ = errors(level, rgb_gt)
    e = e0 if bound is None else torch.min(e0, bound.unsqueeze(-1).to(dt))
    unmasked = e
    if ignore:
        e = e * keep
    ranked = e
    if mutant == "rank_before_keep":
        ranked = unmasked
    elif mutant == "rank_before_bound":
        ranked = e0 * keep if ignore else e0
    flat = ranked.detach().reshape(b, -1)
    if mutant == "upper_median":
        thr = flat.sort(-1).values[:, flat.shape[1] // 2]
    else:
        thr = torch.median(flat, dim=-1)[0]
    t5 = thr.view(-1, 1, 1, 1, 1)
    sel = e < t5 if mutant == "strict_less" else e <= t5
    kept = int(sel.sum())
    rgb_loss = e[sel].mean()
    if mutant == "mask_at_receiver":
        # the value is the reference's; the gradient is that of (sum of ALL e) / count, cut off at the receiving pixels that are dropped
        total = e.sum() / kept
        g, = torch.autograd.grad(total, level["rgb"], retain_graph=True)
        g = g * sel.unsqueeze(-1).to(dt)
        rgb_loss = rgb_loss.detach() + ((level["rgb"] - level["rgb"].detach()) * g).sum()
    loss = rgb_loss * config.get("lambda_coarse", 1) + rgb_loss * config.get("lambda_fine", 1)
    out = dict(loss_rgb=rgb_loss, thresholds=thr.detach(), kept=kept, keep=keep.squeeze(-1), e=e.detach().squeeze(-1))
    if lam_eas > 0:
        eas = OL.edge_aware_smoothness(rgb_gt.unsqueeze(-2), level["depth"])
        if ignore:
            eas = eas * (1 - torch.ceil(F.interpolate(invalid.squeeze(-1).to(dt), size=level["depth"].shape[-2:])))
        eas = eas.mean()
        loss = loss + eas * lam_eas
        out["loss_eas"] = eas
    out["loss_invalid_ratio"] = invalid.to(dt).mean()
    return loss, out


def to_double(level, rgb_gt, bound=None):
    """the same inputs as doubles (the exact fp32 values): the fp64 yardstick"""
    lv = {k: (v.double() if v.is_floating_point() else v) for k, v in level.items()}
    return lv, rgb_gt.double(), None if bound is None else bound.double()
