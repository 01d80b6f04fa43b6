"""Generates tests/golden/loss_pixel.npz FROM THE REAL REFERENCE: seeded tensors in the layout the ray samplers' reconstruct() returns, fed
straight to the reference's ReconstructionLoss (models/bts/model/loss.py) for the settings `native_pixel_loss: true` opens: criterion l1,
l2 (the reference's defaults), l1 + median (strict), l2 + median (weight_guided), l2 + weight_guided_diverse, l1+ssim +
weight_guided_diverse, each with lambda_edge_aware_smoothness = 0.01, on four layouts (tests/_loss_pixel_oracle.py: LAYOUTS, CONFIGS).
Stores, per layout, the inputs in a compact EXACT form (_loss_pixel_oracle.load_inputs) and, per layout and config, the loss, the loss
dict, the per-sample thresholds, the kept count and d loss / d rgb, d loss / d depth.

The inputs carry, by construction: two views that are exact copies of each other on a block of h / 2 x w pixels in the red and green
channels (the amin tie of the per-channel criteria, whose minimum over the views is per channel: two channels tie, the third does not.
Blue differs on purpose: the shipped l1+ssim kernels, which serve l1+ssim + diverse unchanged, give a pixel whose two best views tie
EXACTLY to the first of them -- their tests keep every pixel's two smallest e_v apart -- and a copy in all three channels ties e_v
exactly wherever SSIM's clamp saturates in both views; with blue apart the L1 part of e_v differs and nothing ties); in sample 0 a plateau of
equal errors around the median's rank (the <= tie); samples with clearly different medians; in layout "odd" one sample with more than
half of its rays invalid (threshold 0) and fewer than half everywhere else.  The script ASSERTS, on the fp32 reference: every (ray, view)
is further than 1e-4 from both comparisons of the diverse rule (no ray is ever set aside in a comparison); the restatement in
tests/_loss_pixel_oracle.py reproduces the reference; and each of its mutants moves the stored loss or a gradient beyond the tests' bars.

    python -B tests/golden/gen_golden_loss_pixel.py      (build container only)"""
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
from tests import _loss_pixel_oracle as PO

torch.set_num_threads(4)

BAR_LOSS, BAR_GRAD = 1e-5, 1e-4        # the GPU tests' bars: loss absolute, gradients relative to the largest entry
# which configs a mutant must move (on at least one layout each)
MUTANT_CONFIGS = {"upper_median": ("l1_median", "l2_median"), "strict_less": ("l1_median", "l2_median"),
                  "first_tie": ("l1", "l2", "l1_median", "l2_median", "l2_diverse"), "min_after_mean": ("l1", "l2", "l1_median", "l2_median", "l2_diverse"),
                  "biased_std": ("l2_diverse", "l1ssim_diverse")}


def compact_inputs(name, n, pc, h, w, nv, K, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=g)
    a, b = (h * 35) // 100, (h * 65 + 99) // 100                 # rows [a, b): the plateau of sample 0
    gt_f = F.avg_pool2d(torch.rand(n * pc, 3, h + 4, w + 4, generator=g), 3, 1, 1)[:, :, 2:-2, 2:-2]
    gt_u8 = (16 + gt_f * 184).round().reshape(n, pc, 3, h, w).permute(0, 1, 3, 4, 2).contiguous().to(torch.int64)      # k / 256 in [1/16, 25/32]
    gt16 = gt_u8 * 256                                                                                          # in the renders' k / 65536
    rgb = torch.empty(n, pc, h, w, nv, 3, dtype=torch.int64)
    for s in range(n):
        for v in range(nv):
            sigma = 0.03 * (1 + 2 * s) * (1 + 0.5 * v)
            rgb[s, :, :, :, v] = gt16[s] + (torch.randn(pc, h, w, 3, generator=g) * sigma * 65536).round().to(torch.int64)
    # sample 0: small errors above the plateau, ONE exact error 1 / 8 on it (view 0, every channel; the other views further off), large
    # errors below
    rgb[0, :, :a] = gt16[0, :, :a].unsqueeze(-2) + ri(-3276, 3277, pc, a, w, nv, 3)
    rgb[0, :, a:b] = gt16[0, :, a:b].unsqueeze(-2) + 8192 + ri(200, 3000, pc, b - a, w, nv, 3)
    rgb[0, :, a:b, :, 0] = gt16[0, :, a:b] + 8192
    big = ri(19661, 26215, pc, h - b, w, nv, 3)                                                                # 0.3 .. 0.4
    rgb[0, :, b:] = gt16[0, :, b:].unsqueeze(-2) + torch.where(gt16[0, :, b:].unsqueeze(-2) < 32768, big, -big)
    if nv > 1:
        rgb[:, 0, : h // 2, :, 1, :2] = rgb[:, 0, : h // 2, :, 0, :2]                                           # the amin tie
    rgb = rgb.clamp(0, 65535)
    depth = torch.rand(n, pc, h, w, generator=g) * 100 + 0.5
    depth[:, pc - 1, 0, 0] = 1e-4
    wts = ri(1, 256, n, pc, h, w, K)
    inv = torch.zeros(n, pc, h, w, K, nv, dtype=torch.uint8)
    inv[:, :, 0] = 1                                           # row 0: every sample of every view
    inv[:, :, 2, :3, : K // 2, 0] = 1                          # part of view 0's mass
    inv[:, :, 2, w - 3:, 0, :] = 1                             # one sample of every view: strict calls it invalid, the weights do not
    if name == "odd":
        inv[n - 1, :, (2 * h) // 5:] = 1                       # more than half of the last sample's rays
    samps = ri(0, 4, n, pc, h, w, K, nv, 3)
    samps[:, :, 1, : w // 2] = samps[:, :, 1, : w // 2, :1].clone()                     # no diversity in any view
    samps[:, :, 1, w // 2:, :, 0] = samps[:, :, 1, w // 2:, :1, 0].clone()              # ... in view 0 only
    marginal = torch.zeros(n, pc, h, w, dtype=torch.bool)
    marginal[:, :, h - 1, w // 2:] = True                                       # unbiased std just above .01, biased std below
    zk = torch.arange(K, dtype=torch.float64) - (K - 1) / 2
    zk = zk / zk.std(unbiased=True)
    base = samps[marginal][:, :1].float() / 4
    marg = (base.double() + 0.0105 * zk.view(1, K, 1, 1)).float().contiguous()
    return {f"{name}_rgb_gt_u8": gt_u8.numpy().astype(np.uint8), f"{name}_rgb_u16": rgb.numpy().astype(np.uint16),
            f"{name}_depth": depth.numpy(), f"{name}_weights_u8": wts.numpy().astype(np.uint8), f"{name}_invalid": inv.numpy(),
            f"{name}_rgb_samps_u2": samps.numpy().astype(np.uint8), f"{name}_marginal": marginal.numpy(),
            f"{name}_rgb_samps_marginal": marg.numpy()}


def run(loss_fn, level, gt):
    lv = dict(level)
    lv["rgb"], lv["depth"] = level["rgb"].clone().requires_grad_(True), level["depth"].clone().requires_grad_(True)
    loss, parts = loss_fn(lv, gt)
    g_rgb, g_depth = torch.autograd.grad(loss, [lv["rgb"], lv["depth"]])
    return loss.detach(), parts, g_rgb, g_depth


def moved(a, b):
    """does result b differ from the stored result a beyond the tests' bars?"""
    return (abs(a[0].item() - b[0].item()) > BAR_LOSS or (a[2] - b[2]).abs().max().item() > BAR_GRAD * a[2].abs().max().item())


def main():
    ref = load_reference()
    arrays, caught = {}, {m: set() for m in PO.MUTANTS}
    for name, (n, pc, h, w, nv, K) in PO.LAYOUTS.items():
        comp = compact_inputs(name, n, pc, h, w, nv, K, seed=1600 + h)
        arrays.update(comp)
        level, gt = PO.load_inputs(comp, name)
        wsum, std = PO.diverse_stats(level)
        assert ((std - 0.01).abs() > 1e-4).all() and ((wsum - 0.9).abs() > 1e-4).all(), "a (ray, view) sits on a comparison of the diverse rule"
        _, std_b = PO.diverse_stats(level, "biased_std")
        assert ((std_b - 0.01).abs() > 1e-4).all() and ((std_b < 0.01) != (std < 0.01)).any()
        if nv > 1:      # l1+ssim: every pixel's two smallest e_v are more than 1e-6 apart (the contract of the shipped kernels, see the docstring)
            two = PO.OL.errors_l1ssim(level["rgb"], gt.unsqueeze(-2)).squeeze(-1).sort(-1).values[..., :2]
            assert ((two[..., 1] - two[..., 0]) > 1e-6).all(), "two views (nearly) tie under l1+ssim"
            print(name, "smallest gap between the two best views under l1+ssim", (two[..., 1] - two[..., 0]).min().item())
        for cname in PO.CONFIGS:
            cfg = PO.config_of(cname)

            def ref_fn(lv, g):
                return ref.ReconstructionLoss(dict(cfg))(dict(coarse=[lv], fine=[dict(lv)], rgb_gt=g))
            want = run(ref_fn, level, gt)
            got = run(lambda lv, g: PO.reconstruction_loss(lv, g, cfg), level, gt)
            assert abs(want[0].item() - got[0].item()) <= 1e-6, (name, cname, want[0], got[0])
            for x, y in ((want[2], got[2]), (want[3], got[3])):
                assert (x - y).abs().max().item() <= 1e-5 * x.abs().max().item(), (name, cname)
            o = got[1]
            frac = 1 - o["keep"].reshape(n, -1).mean(-1)
            if name == "odd" and PO.CONFIGS[cname].get("invalid_policy", "strict") != "none":
                assert frac[-1] > 0.5 and (frac[:-1] < 0.5).all()
            else:
                assert (frac < 0.5).all()
            thr, kept = o["thresholds"], o["kept"]
            if thr is not None:
                assert thr[0].item() == (0.125 if "l1" in cname else 0.015625), (name, cname, thr)      # the plateau holds sample 0's median
                assert (thr[:-1] > 0).all() and ((thr[-1] == 0) == (name == "odd")), (name, cname, thr)
                assert len(set(thr.tolist())) == n                                                       # clearly different medians
            for m, cfgs in MUTANT_CONFIGS.items():
                if cname in cfgs and moved(want, run(lambda lv, g: PO.reconstruction_loss(lv, g, cfg, mutant=m), level, gt)):
                    caught[m].add((cname, name))
            key = f"{name}_{cname}"
            arrays.update({f"{key}_loss": want[0].reshape(1).numpy(),
                           f"{key}_loss_dict": np.array([float(want[1][k]) for k in PO.DICT_KEYS], dtype=np.float64),
                           f"{key}_thresholds": (thr if thr is not None else torch.zeros(0)).numpy(),
                           f"{key}_kept": np.array([kept if kept is not None else 3 * n * pc * h * w], dtype=np.int64),
                           f"{key}_g_rgb": want[2].numpy(), f"{key}_g_depth": want[3].numpy()})
            print(name, cname, "loss", want[0].item(), "thr", None if thr is None else thr.tolist(), "kept", kept)
    for m, cfgs in MUTANT_CONFIGS.items():
        hit = {c for c, _ in caught[m]}
        print("mutant", m, "moves", sorted(caught[m]))
        assert hit == set(cfgs), f"mutant {m} is not caught under {sorted(set(cfgs) - hit)}"
    out = os.path.join(HERE, "loss_pixel.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1_000_000


if __name__ == "__main__":
    main()
