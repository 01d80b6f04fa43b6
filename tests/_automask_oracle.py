"""TEST INFRASTRUCTURE: CPU restatement of the reference's auto-masking -- the trainer's error map (models/bts/trainer.py:201-206) and
ReconstructionLoss(conf, use_automasking=True) (models/bts/model/loss.py:139-143, 157-158, 174-175) for one scale with the fine dict
aliased to the coarse one.  Pinned to the REAL reference by tests/golden/automask.npz (tests/golden/gen_golden_automask.py) in
tests/test_automask_cpu.py.

``mutant`` swaps ONE of the reference's quirks for the plausible wrong reading; the golden's generator asserts that each of them moves
a stored map, loss or gradient beyond the tests' bars:
    no_second_half       the frames, already in [0, 1], are NOT halved again before the comparison
    no_self              a loss frame's comparison with itself is left out of its mean
    reflection           reflection padding instead of zero padding at the frame border
    thresh_channel_mean  l1 / l2: the bound is compared with the mean over the channels instead of with each channel
    thresh_after_median  the median ranking sees the unbounded errors
    tie_full             e == thresh hands the whole gradient to e instead of torch.min's half"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import bts_loss as OL
from tests import _loss_pixel_oracle as PO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "automask.npz")
# the error map: (n, v, H, W, ids_loss)
MAP_CASES = {"tiles": (2, 4, 33, 70, [0, 2]), "one": (1, 3, 19, 35, [1]), "repeat": (1, 8, 24, 40, [3, 0, 3, 5]), "tiny": (1, 2, 3, 5, [0, 1])}
MAP_MUTANTS = ("no_second_half", "no_self", "reflection")
# the loss: (n, pc, h, w, nv, K); p8: the wave kernel, p16 / ragged: the tiled one, median: the pixel kernel's median per sample
LAYOUTS = {"p8": (2, 3, 8, 8, 3, 4), "p16": (2, 2, 16, 16, 2, 4), "ragged": (2, 2, 12, 20, 3, 4), "median": (3, 2, 8, 8, 2, 4)}
LAMBDA_EAS = 0.01
CONFIGS = {
    "ssim_wg": dict(criterion="l1+ssim", invalid_policy="weight_guided"),
    "ssim_strict_lean": dict(criterion="l1+ssim", invalid_policy="strict"),        # the HIP side gets invalid_any instead of invalid
    "l2": dict(criterion="l2", invalid_policy="strict"),
    "l1_median": dict(criterion="l1", invalid_policy="strict", median_thresholding=True),
    "l2_diverse": dict(criterion="l2", invalid_policy="weight_guided_diverse"),
}
LOSS_MUTANTS = ("thresh_channel_mean", "thresh_after_median", "tie_full")
DICT_KEYS = PO.DICT_KEYS
TIE = {"l1": 0.125, "l2": 0.015625}        # the error of view 0 in the constructed block (1 / 8 off in every channel)


def config_of(name):
    return dict(CONFIGS[name], lambda_edge_aware_smoothness=LAMBDA_EAS)


def crit_key(cname):
    """which of the golden's three threshold maps a configuration reads"""
    c = CONFIGS[cname]["criterion"]
    return "ssim" if c == "l1+ssim" else c


def map_frames(z, case):
    """the golden's 8-bit frames -> (n, v, 3, H, W) float32 in [0, 1) (k / 256: exact)"""
    return torch.from_numpy(z[f"map_{case}_u8"].astype(np.float32)) / 256


def load_inputs(z, layout):
    """-> (level, rgb_gt (n, pc, h, w, 3)) in _loss_pixel_oracle's compact exact storage"""
    return PO.load_inputs(z, f"am_{layout}")


def load_thresh(z, layout, cname):
    """(n, pc, h, w) float32: the seeded map, with the exact ties of the constructed block for l1 / l2"""
    return torch.from_numpy(z[f"am_{layout}_thresh_{crit_key(cname)}"])


def _ssim(x, y, reflect):
    if not reflect:
        return OL.ssim_comp(x, y)
    x, y = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
    mu_x, mu_y = OL._gauss(x), OL._gauss(y)
    sigma_x, sigma_y, sigma_xy = OL._gauss(x ** 2) - mu_x ** 2, OL._gauss(y ** 2) - mu_y ** 2, OL._gauss(x * y) - mu_x * mu_y
    n = (2 * mu_x * mu_y + 0.01 ** 2) * (2 * sigma_xy + 0.03 ** 2)
    d = (mu_x ** 2 + mu_y ** 2 + 0.01 ** 2) * (sigma_x + sigma_y + 0.03 ** 2)
    return torch.clamp(1 - n / d, 0, 1) / 2


def error_map(images_ip, ids_loss, mutant=None):
    """trainer.py:203-205: images_ip (n, v, 3, h, w) in [0, 1] -> errors (n, v, 1, h, w), in images_ip's dtype"""
    n, v, c, h, w = images_ip.shape
    ids = [int(i) for i in ids_loss]
    L = len(ids)
    s = 1.0 if mutant == "no_second_half" else .5
    x = (images_ip * s).unsqueeze(2).expand(-1, -1, L, -1, -1, -1).reshape(n * v * L, c, h, w)          # frame f against ...
    y = (images_ip[:, ids] * s).unsqueeze(1).expand(-1, v, -1, -1, -1, -1).reshape(n * v * L, c, h, w)  # ... loss frame j
    e = .85 * torch.mean(_ssim(x, y, mutant == "reflection"), dim=1) + .15 * torch.mean(torch.abs(x - y), dim=1)
    e = e.view(n, v, L, h, w)
    if mutant == "no_self":
        other = torch.tensor([[float(f != j) for j in ids] for f in range(v)], dtype=e.dtype).view(1, v, L, 1, 1)
        return ((e * other).sum(2) / other.sum(2).clamp_min(1)).unsqueeze(2)
    return e.mean(2).unsqueeze(2)


def images4(images_ip, ids_loss):
    """trainer.py:206"""
    return torch.cat((images_ip, error_map(images_ip, ids_loss)), dim=2)


def errors_before_bound(level, rgb_gt, config):
    """-> the per-pixel errors after the minimum over the views, before the bound: (n, pc, h, w, 1) for l1+ssim, (..., 3) for l1 / l2"""
    crit = config.get("criterion", "l2")
    gt = rgb_gt.unsqueeze(-2)
    if crit == "l1+ssim":
        return OL.errors_l1ssim(level["rgb"], gt).amin(-2)
    d = level["rgb"] - gt
    return (d.abs() if crit == "l1" else d * d).amin(-2)


def reconstruction_loss(level, rgb_gt4, config, mutant=None):
    """loss.py:83-293 with use_automasking=True.  level: a render dict in reconstruct()'s layout with the RENDERED rgb (n, pc, h, w, nv, 3)
    (the reference's fourth rendered channel is cut off first thing: it is not an input here); rgb_gt4 (n, pc, h, w, 4)
    -> (loss, dict(loss_rgb, loss_eas, loss_invalid_ratio, thresholds, kept, keep, bound share))"""
    crit = config.get("criterion", "l2")
    policy = config.get("invalid_policy", "strict")
    ignore = policy not in (None, "none")
    median = config.get("median_thresholding", False)
    lam_eas = config.get("lambda_edge_aware_smoothness", 0)
    thresh, rgb_gt = rgb_gt4[..., -1:], rgb_gt4[..., :-1]
    b = level["rgb"].shape[0]
    invalid = PO.invalid_rays(level, policy if ignore else "none")
    keep = 1 - invalid.to(torch.float32)
    e0 = errors_before_bound(level, rgb_gt, config)
    if mutant == "thresh_channel_mean" and crit != "l1+ssim":
        e = torch.min(e0.mean(-1, keepdim=True), thresh).expand(e0.shape)
    elif mutant == "tie_full":
        e = torch.where(e0 <= thresh, e0, thresh.expand(e0.shape))
    else:
        e = torch.min(e0, thresh)
    if ignore:
        e = e * keep
    thr = kept = None
    if median:
        ranked = (e0 * keep if ignore else e0) if mutant == "thresh_after_median" else e
        thr = torch.median(ranked.reshape(b, -1), dim=-1)[0]
        sel = ranked <= thr.view(-1, 1, 1, 1, 1)
        e = e[sel]
        kept = int(sel.sum())
    rgb_loss = e.mean()
    loss = rgb_loss * config.get("lambda_coarse", 1) + rgb_loss * config.get("lambda_fine", 1)
    out = dict(loss_rgb=rgb_loss, thresholds=None if thr is None else thr.detach(), kept=kept, keep=keep.squeeze(-1),
               bound=(e0.detach() > thresh).float().mean().item())
    if lam_eas > 0:
        eas = OL.edge_aware_smoothness(rgb_gt.unsqueeze(-2), level["depth"])
        if ignore:
            eas = eas * (1 - torch.ceil(F.interpolate(invalid.squeeze(-1).to(torch.float32), size=level["depth"].shape[-2:])))
        eas = eas.mean()
        loss = loss + eas * lam_eas
        out["loss_eas"] = eas
    out["loss_invalid_ratio"] = invalid.float().mean()
    return loss, out
