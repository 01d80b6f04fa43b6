"""TEST INFRASTRUCTURE: CPU restatement of the reference's ReconstructionLoss (models/bts/model/loss.py:83-293) for the settings the
opt-in `native_pixel_loss: true` opens -- criterion l1 / l2 with or without median_thresholding under the four invalid-ray policies, and
l1+ssim under weight_guided_diverse -- for one scale, with the fine dict aliased to the coarse one (trainer.py:247-248).  Pinned to the
REAL reference by tests/golden/loss_pixel.npz (tests/golden/gen_golden_loss_pixel.py) in tests/test_loss_pixel_cpu.py.

``mutant`` swaps ONE of the reference's quirks for the plausible wrong reading; the golden's generator asserts that each of them moves
the loss or a gradient beyond the test's bars:
    upper_median    rank N / 2 instead of torch.median's lower (N - 1) / 2
    strict_less     e < thr instead of e <= thr
    first_tie       the first view at the minimum takes the whole gradient instead of amin's equal split
    min_after_mean  the minimum over the views of the channel MEAN instead of per channel
    biased_std      std over K instead of K - 1 in the diverse flags"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import bts_loss as OL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_pixel.npz")
LAYOUTS = {"p8": (2, 3, 8, 8, 3, 5), "odd": (3, 2, 17, 23, 2, 5), "frame": (1, 2, 40, 72, 3, 5), "one": (1, 1, 9, 8, 1, 3)}   # (n, pc, h, w, nv, K)
LAMBDA_EAS = 0.01
CONFIGS = {
    "l1": dict(criterion="l1", invalid_policy="none"),
    "l2": dict(),                                                     # the reference's defaults: criterion l2, invalid_policy strict
    "l1_median": dict(criterion="l1", invalid_policy="strict", median_thresholding=True),
    "l2_median": dict(criterion="l2", invalid_policy="weight_guided", median_thresholding=True),
    "l2_diverse": dict(criterion="l2", invalid_policy="weight_guided_diverse"),
    "l1ssim_diverse": dict(criterion="l1+ssim", invalid_policy="weight_guided_diverse"),
}
DICT_KEYS = ["loss_rgb_coarse", "loss_rgb_fine", "loss_eas", "loss_invalid_ratio", "loss"]
MUTANTS = ("upper_median", "strict_less", "first_tie", "min_after_mean", "biased_std")


def config_of(name):
    return dict(CONFIGS[name], lambda_edge_aware_smoothness=LAMBDA_EAS)


def load_inputs(z, layout):
    """The golden's compact storage -> the float32 tensors the reference was fed (every step below is exact in fp32, so the generator
    and the tests see the same bits): ground truth as k / 256, renders as k / 65536, sample colours as k / 4 with the marginal rays'
    colours stored as floats, weights as integer draws normalised per ray."""
    g = lambda k: torch.from_numpy(z[f"{layout}_{k}"])
    f = lambda k: torch.from_numpy(z[f"{layout}_{k}"].astype(np.float32))
    gt = f("rgb_gt_u8") / 256
    rgb = f("rgb_u16") / 65536
    samps = f("rgb_samps_u2") / 4
    m = g("marginal").bool()
    samps[m] = g("rgb_samps_marginal")
    q = f("weights_u8")
    return dict(rgb=rgb, depth=g("depth"), weights=q / q.sum(-1, keepdim=True), invalid=g("invalid").float(), rgb_samps=samps), gt


def diverse_stats(level, mutant=None):
    """-> (sum_k invalid w, mean_c std_k(rgb_samps)) per (ray, view)"""
    wsum = (level["invalid"].to(torch.float32) * level["weights"].unsqueeze(-1)).sum(-2)
    std = torch.std(level["rgb_samps"], dim=-3, unbiased=mutant != "biased_std").mean(-1)
    return wsum, std


def invalid_rays(level, policy, mutant=None):
    """loss.py:100-121 -> bool (n, pc, h, w, 1)"""
    inv, wts = level["invalid"], level["weights"]
    if policy == "strict":
        return torch.all(torch.any(inv > .5, dim=-2), dim=-1).unsqueeze(-1)
    if policy == "weight_guided":
        return torch.all((inv.to(torch.float32) * wts.unsqueeze(-1)).sum(-2) > .9, dim=-1, keepdim=True)
    if policy == "weight_guided_diverse":
        wsum, std = diverse_stats(level, mutant)
        return torch.all((wsum > .9) | (std < 0.01), dim=-1, keepdim=True)
    return torch.zeros(inv.shape[:-2] + (1,), dtype=torch.bool)


def reconstruction_loss(level, rgb_gt, config, mutant=None):
    """-> (loss, dict(loss_rgb, loss_eas, loss_invalid_ratio, thresholds (n) | None, kept | None, keep (n, pc, h, w)))"""
    crit = config.get("criterion", "l2")
    policy = config.get("invalid_policy", "strict")
    ignore = policy not in (None, "none")
    median = config.get("median_thresholding", False)
    lam_eas = config.get("lambda_edge_aware_smoothness", 0)
    rgb, gt = level["rgb"], rgb_gt.unsqueeze(-2)
    b = rgb.shape[0]
    invalid = invalid_rays(level, policy if ignore else "none", mutant)
    keep = 1 - invalid.to(torch.float32)
    if crit == "l1+ssim":
        e = OL.errors_l1ssim(rgb, gt)
    else:
        d = rgb - gt
        e = d.abs() if crit == "l1" else d * d
    if mutant == "min_after_mean" and crit != "l1+ssim":
        e = e.mean(-1, keepdim=True).amin(-2).expand(e.shape[:-2] + (3,))
    elif mutant == "first_tie":
        e = e.min(-2).values
    else:
        e = e.amin(-2)
    if ignore:
        e = e * keep
    thr = kept = None
    if median:
        flat = e.reshape(b, -1)
        if mutant == "upper_median":
            thr = flat.sort(-1).values[:, flat.shape[1] // 2]
        else:
            thr = torch.median(flat, dim=-1)[0]
        sel = e < thr.view(-1, 1, 1, 1, 1) if mutant == "strict_less" else e <= thr.view(-1, 1, 1, 1, 1)
        e = e[sel]
        kept = int(sel.sum())
    rgb_loss = e.mean()
    loss = rgb_loss * config.get("lambda_coarse", 1) + rgb_loss * config.get("lambda_fine", 1)
    out = dict(loss_rgb=rgb_loss, thresholds=None if thr is None else thr.detach(), kept=kept, keep=keep.squeeze(-1))
    if lam_eas > 0:
        eas = OL.edge_aware_smoothness(gt, level["depth"])
        if ignore:
            eas = eas * (1 - torch.ceil(F.interpolate(invalid.squeeze(-1).to(torch.float32), size=level["depth"].shape[-2:])))
        eas = eas.mean()
        loss = loss + eas * lam_eas
        out["loss_eas"] = eas
    out["loss_invalid_ratio"] = invalid.float().mean()
    return loss, out


def eas_fp64(rgb_gt, depth, keep):
    """The masked smoothness term's SUM over the rays and its gradient w.r.t. depth, evaluated in fp64 (the yardstick that measures an
    fp32 kernel's own error)."""
    d = depth.double().clone().requires_grad_(True)
    s = (OL.edge_aware_smoothness(rgb_gt.double().unsqueeze(-2), d) * keep.double()).sum()
    g, = torch.autograd.grad(s, d)
    return s.detach(), g
