"""Generates tests/golden/loss_frames.npz FROM THE REAL REFERENCE: seeded tensors in the layout the ray samplers' reconstruct() returns,
fed straight to the reference's ReconstructionLoss (models/bts/model/loss.py) for patches LARGER than the shipped configs' 8 x 8 -- the
trainer's default 16 x 16 patch and a small whole frame (ImageRaySampler.reconstruct: pc = rendered views, (h, w) = frame).
Config: l1+ssim, weight_guided, lambda_edge_aware_smoothness = 0.01.  Stores, per layout, the inputs (invalid as uint8), the loss, the
loss dict and d loss / d rgb, d loss / d depth.

    python -B tests/golden/gen_golden_loss_frames.py      (build container only)"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn.functional as F

from oracle.ref_shim import load_reference

torch.set_num_threads(4)

LAYOUTS = {"patch16": (2, 3, 16, 16, 3, 5), "frame": (1, 2, 40, 72, 3, 5)}      # (n, pc, h, w, nv, K)
CONFIG = dict(criterion="l1+ssim", invalid_policy="weight_guided", lambda_edge_aware_smoothness=0.01)
DICT_KEYS = ["loss_rgb_coarse", "loss_rgb_fine", "loss_eas", "loss_invalid_ratio", "loss"]


def inputs(n, pc, h, w, nv, K, seed):
    """Correlated ground truth, noisy renders with one exact-match view, depths beyond the [1e-3, 80] clamp, a band of invalid rays."""
    g = torch.Generator().manual_seed(seed)
    gt = F.avg_pool2d(torch.rand(n * pc, 3, h + 4, w + 4, generator=g), 3, 1, 1)[:, :, 2:-2, 2:-2]
    gt = gt.reshape(n, pc, 3, h, w).permute(0, 1, 3, 4, 2).contiguous()
    rgb = (gt.unsqueeze(-2) + 0.15 * torch.randn(n, pc, h, w, nv, 3, generator=g)).clamp(0, 1)
    rgb[:, 0, :, :, 0] = gt[:, 0]
    depth = torch.rand(n, pc, h, w, generator=g) * 100 + 0.5
    depth[:, 1, 0, 0] = 1e-4
    wts = torch.rand(n, pc, h, w, K, generator=g)
    wts = wts / wts.sum(-1, keepdim=True)
    inv = (torch.rand(n, pc, h, w, K, nv, generator=g) < 0.3).float()
    inv[:, :, 0, :, :, :] = 1.0
    inv[:, :, 1, :, : K // 2, 0] = 0.0
    return rgb, depth, wts, inv, gt


def main():
    ref = load_reference()
    arrays = {}
    for name, (n, pc, h, w, nv, K) in LAYOUTS.items():
        rgb, depth, wts, inv, gt = inputs(n, pc, h, w, nv, K, seed=1300 + h)
        rgb.requires_grad_(True), depth.requires_grad_(True)
        level = dict(rgb=rgb, depth=depth, weights=wts, invalid=inv)
        crit = ref.ReconstructionLoss(dict(CONFIG))
        loss, parts = crit(dict(coarse=[level], fine=[dict(level)], rgb_gt=gt))
        g_rgb, g_depth = torch.autograd.grad(loss, [rgb, depth])
        arrays.update({f"{name}_rgb": rgb.detach().numpy(), f"{name}_depth": depth.detach().numpy(), f"{name}_weights": wts.numpy(),
                       f"{name}_invalid": inv.numpy().astype(np.uint8), f"{name}_rgb_gt": gt.numpy(),
                       f"{name}_loss": loss.detach().reshape(1).numpy(),
                       f"{name}_loss_dict": np.array([float(parts[k]) for k in DICT_KEYS], dtype=np.float64),
                       f"{name}_g_rgb": g_rgb.numpy(), f"{name}_g_depth": g_depth.numpy()})
        print(name, "loss", loss.item(), {k: float(parts[k]) for k in DICT_KEYS})
    meta = dict(layouts=LAYOUTS, config=CONFIG, dict_keys=DICT_KEYS)
    out = os.path.join(HERE, "loss_frames.npz")
    np.savez_compressed(out, meta=np.array(repr(meta)), **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
