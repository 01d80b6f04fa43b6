"""Generates tests/golden/loss_ssim_median.npz FROM THE REAL REFERENCE, on the CPU: seeded tensors in the layout the ray samplers'
reconstruct() returns, fed to the reference's ReconstructionLoss (models/bts/model/loss.py) with criterion l1+ssim AND
median_thresholding, lambda_edge_aware_smoothness = 0.01, for the five configurations and four layouts of
tests/_loss_ssim_median_oracle.py (weight_guided; strict, which the HIP side is fed lean; none; weight_guided_diverse; weight_guided with
use_automasking and a seeded bound map).  Stores, per layout, the inputs in the compact EXACT form of _loss_pixel_oracle.load_inputs, the
bound map and D = the largest |e_fp32 - e_fp64| of the reference's own compute_errors_l1ssim(...).amin(-2) (the same function on the
same values as doubles); per layout and configuration the loss, the loss dict, the per-sample thresholds of the fp32 reference and of its
fp64 evaluation, the kept count and d loss / d rgb, d loss / d depth.

THE CONSTRUCTION.  A HIP kernel's e is not bit-equal to the reference's (SSIM sums in another order), so a pixel just above a threshold
could be kept on one side and dropped on the other.  The inputs therefore put every sample's errors in TWO populations with nothing in
between, the lower one holding exactly rank + 1 = (N - 1) // 2 + 1 pixels, so that the median is the largest error of the lower
population and the next error above it is far away:
  - a seeded sweep (by columns or by rows, per sample) marks pixels as `hard`: every view's colours there are 0.2 .. 0.4 off the ground
    truth, to a random side; everywhere else every view is the ground truth plus small noise.  The 3 x 3 SSIM window carries a hard pixel's error to its
    eight neighbours, so the upper population is the DILATION of the hard set; the sweep stops where that dilation has exactly N // 2
    pixels.  "ragged": sample 0 is swept by columns, the kept / dropped border of patch 1 lies on the tile border x = 16 and that of
    patch 0 inside a tile; sample 1 by rows, the border inside a tile.  "frame": one patch over 15 tiles, swept by columns;
  - "p8", sample 0: patch 1 is an exact copy of patch 0 in every input and the dilation has N // 2 - 1 pixels, so the lower population has
    rank + 2 pixels whose two largest are equal: the value at the median's rank also sits one rank above it (asserted), kept = rank + 2;
  - invalid rays (of every policy: all samples of all views; one sample of all views = strict only; no diversity in any view = diverse
    only; and view 0 alone, which no policy calls invalid) lie in the LOWER population, where they rank as zeros without moving the count;
  - "odd", last sample: most of the lower population and a fifth of the upper one is invalid under every policy -- more than half of the
    sample, threshold 0, only zeros kept; the lower population's valid rest is what `rank_before_keep` keeps wrongly;
  - the bound map of the automasking configuration binds part of the lower population below its largest unbounded error, leaves the upper
    population above it, and bounds a few pixels of the upper population to a value between the two (what `rank_before_bound` keeps wrongly).
The script ASSERTS on the fp32 reference, per layout, configuration and sample: the smallest error strictly above the threshold exceeds
it by at least 20 D; every pixel's two smallest e_v are more than 1e-6 apart; no |e - bound| is below 20 D; no (ray, view) is within 1e-4
of a comparison of the diverse rule; the restatement reproduces the reference; each mutant moves the stored loss, kept count or a gradient
beyond the tests' bars on at least one layout.

    python -B tests/golden/gen_golden_loss_ssim_median.py      (build container only)"""
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
from tests import _loss_ssim_median_oracle as MO

torch.set_num_threads(4)

BAR_LOSS, BAR_GRAD = 1e-5, 1e-4        # the GPU tests' bars: loss absolute, gradients relative to the largest entry
SEEDS = {"p8": 2108, "ragged": 2120, "odd": 2117, "frame": 2140}       # the committed seeds (searched: main() asserts, it does not search)
MUTANT_CONFIGS = {"upper_median": tuple(MO.CONFIGS), "strict_less": tuple(MO.CONFIGS), "mask_at_receiver": tuple(MO.CONFIGS),
                  "rank_before_keep": ("wg", "strict_lean", "diverse", "wg_automask"), "rank_before_bound": ("wg_automask",)}


def dilate(m):
    """(n, pc, h, w) bool -> the pixels with a marked pixel in their 3 x 3 neighbourhood inside the patch"""
    n, pc, h, w = m.shape
    return F.max_pool2d(m.reshape(n * pc, 1, h, w).float(), 3, 1, 1).reshape(n, pc, h, w) > 0


def sweep(pc, h, w, by_rows, target, twin=False, pre=None):
    """marks pixels of one sample in sweep order (columns left to right, or rows top to bottom, through every patch in turn) until the
    dilation of the marked set has exactly `target` pixels.  twin: patches 0 and 1 are marked alike.  pre: (patch, columns) marked
    beforehand, that patch is then left out of the sweep"""
    m = torch.zeros(1, pc, h, w, dtype=torch.bool)
    outer, inner = (h, w) if by_rows else (w, h)
    if pre is not None:
        m[0, pre[0], :, :pre[1]] = True
    for a in range(outer):
        for p in range(1 if twin else 0, pc):
            if pre is not None and p == pre[0]:
                continue
            for b in range(inner):
                y, x = (a, b) if by_rows else (b, a)
                m[0, p, y, x] = True
                if twin and p == 1:
                    m[0, 0, y, x] = True
                c = int(dilate(m).sum())
                if c == target:
                    return m[0]
                assert c < target, ("the sweep steps over the target", c, target)
    raise AssertionError("the sweep never reaches the target")


def compact_inputs(name, n, pc, h, w, nv, K, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=g)
    N = pc * h * w
    gt_f = F.avg_pool2d(torch.rand(n * pc, 3, h + 4, w + 4, generator=g), 3, 1, 1)[:, :, 2:-2, 2:-2]
    gt_u8 = (16 + gt_f * 184).round().reshape(n, pc, 3, h, w).permute(0, 1, 3, 4, 2).contiguous().to(torch.int64)      # k / 256 in [1/16, 25/32]
    gt16 = gt_u8 * 256                                                                                          # in the renders' k / 65536
    hard = torch.zeros(n, pc, h, w, dtype=torch.bool)
    for s in range(n):
        twin = name == "p8" and s == 0
        # "ragged", sample 0: patch 1's hard columns end at x = 14, so its kept / dropped border is the tile border x = 16
        pre = (1, 15) if (name == "ragged" and s == 0) else None
        hard[s] = sweep(pc, h, w, by_rows=(s % 2 == 1), target=N // 2 - (1 if twin else 0), twin=twin, pre=pre)
    upper = dilate(hard)
    rgb = torch.empty(n, pc, h, w, nv, 3, dtype=torch.int64)
    for s in range(n):
        sigma = torch.full((pc, 1, 1, 1, 1), 0.005 * (1 + s))
        if name == "p8" and s == 0:
            sigma[2:] *= 0.4                                     # the lower population's largest error lies in the twin patches
        sigma = sigma * (1 + 0.6 * torch.arange(nv).view(1, 1, 1, nv, 1))       # the views apart: no pixel's two best views tie
        easy = gt16[s].unsqueeze(-2) + (torch.randn(pc, h, w, nv, 3, generator=g) * sigma * 65536).round().to(torch.int64)
        off = ri(13107, 26215, pc, h, w, nv, 3)                                                                 # 0.2 .. 0.4
        y16 = gt16[s].unsqueeze(-2).expand(pc, h, w, nv, 3)
        up = torch.where(y16 - off < 0, True, torch.where(y16 + off > 65535, False, ri(0, 2, pc, h, w, nv, 3).bool()))     # a random side where both fit
        far = y16 + torch.where(up, off, -off)
        rgb[s] = torch.where(hard[s].view(pc, h, w, 1, 1), far, easy)
    rgb = rgb.clamp(0, 65535)
    depth = torch.rand(n, pc, h, w, generator=g) * 100 + 0.5
    depth[:, pc - 1, 0, 0] = 1e-4
    wts = ri(1, 256, n, pc, h, w, K)
    inv = torch.zeros(n, pc, h, w, K, nv, dtype=torch.uint8)
    samps = ri(0, 4, n, pc, h, w, K, nv, 3)
    for s in range(n):
        last_odd = name == "odd" and s == n - 1
        lo = (~upper[s]).nonzero()                              # the lower population in raster order
        for i, (p, y, x) in enumerate(lo.tolist()):
            if last_odd:
                if i % 9 != 4:
                    inv[s, p, y, x] = 1                         # every sample of every view: invalid under every policy
            elif i % 7 == 0:
                inv[s, p, y, x] = 1
            elif i % 7 == 3:
                inv[s, p, y, x, int(wts[s, p, y, x].argmin())] = 1      # one light sample of every view: strict only
            elif i % 7 == 5:
                inv[s, p, y, x, :, 0] = 1                       # view 0 alone: no policy
            elif i % 11 == 1:
                samps[s, p, y, x] = samps[s, p, y, x, :1].clone()       # no diversity in any view: diverse only
        if last_odd:
            for j, (p, y, x) in enumerate(upper[s].nonzero().tolist()):
                if j % 5 == 0:
                    inv[s, p, y, x] = 1
    if name == "p8":
        for t in (gt_u8, rgb, depth, wts, inv, samps):
            t[0, 1] = t[0, 0]
    marginal = torch.zeros(n, pc, h, w, dtype=torch.bool)
    return {f"{name}_rgb_gt_u8": gt_u8.numpy().astype(np.uint8), f"{name}_rgb_u16": rgb.numpy().astype(np.uint16),
            f"{name}_depth": depth.numpy(), f"{name}_weights_u8": wts.numpy().astype(np.uint8), f"{name}_invalid": inv.numpy(),
            f"{name}_rgb_samps_u2": samps.numpy().astype(np.uint8), f"{name}_marginal": marginal.numpy(),
            f"{name}_rgb_samps_marginal": np.zeros((0, K, nv, 3), dtype=np.float32)}, upper


def bound_map(name, e0, upper, D, seed):
    """the per-ray bound (n, pc, h, w) of the automasking configuration (the docstring's construction), on a 2^-20 grid"""
    n, pc, h, w = e0.shape
    g = torch.Generator().manual_seed(seed)
    u = F.avg_pool2d(torch.rand(n * pc, 1, h + 4, w + 4, generator=g), 3, 1, 1)[:, 0, 2:-2, 2:-2].reshape(n, pc, h, w)
    u = (u - u.amin()) / (u.amax() - u.amin())
    t = torch.empty_like(e0)
    for s in range(n):
        lo = e0[s][~upper[s]]
        cap, top = lo.quantile(0.8).item(), lo.max().item()
        assert top - cap > 100 * D, (name, s, cap, top)
        t[s] = torch.where(upper[s], 0.12 + 0.3 * u[s], torch.clamp(lo.median() * (0.25 + 1.5 * u[s]), max=cap))
        between = torch.zeros(pc, h, w, dtype=torch.bool)
        idx = upper[s].nonzero()[2::13]
        between[idx[:, 0], idx[:, 1], idx[:, 2]] = True
        t[s][between] = (cap + top) / 2
    t = (t * 2 ** 20).round() / 2 ** 20
    for _ in range(64):          # away from every compared value: a kernel's rounding must not flip a choice
        near = (e0 - t).abs() <= 40 * D
        if not near.any():
            break
        t = torch.where(near, t + 1.0 / 2 ** 12, t)
    if name == "p8":
        t[0, 1] = t[0, 0]
    assert ((e0 - t).abs() >= 20 * D).all(), name
    return t.float().contiguous()


def run(loss_fn, level, gt):
    lv = dict(level)
    lv["rgb"], lv["depth"] = level["rgb"].clone().requires_grad_(True), level["depth"].clone().requires_grad_(True)
    loss, parts = loss_fn(lv, gt)
    g_rgb, g_depth = torch.autograd.grad(loss, [lv["rgb"], lv["depth"]])
    return loss.detach(), parts, g_rgb, g_depth


def moved(a, b):
    """does result b differ from the stored result a beyond the tests' bars (loss, kept count, d rgb)?"""
    return (abs(a[0].item() - b[0].item()) > BAR_LOSS or a[1]["kept"] != b[1]["kept"]
            or (a[2] - b[2]).abs().max().item() > BAR_GRAD * a[2].abs().max().item())


def main():
    ref = load_reference()
    from models.bts.model.loss import compute_errors_l1ssim
    arrays, caught = {}, {m: set() for m in MO.MUTANTS}
    for name, (n, pc, h, w, nv, K) in MO.LAYOUTS.items():
        comp, upper = compact_inputs(name, n, pc, h, w, nv, K, seed=SEEDS[name])
        level, gt = MO.PO.load_inputs(comp, name)
        N, rank = pc * h * w, (pc * h * w - 1) // 2
        ev32 = compute_errors_l1ssim(level["rgb"], gt.unsqueeze(-2)).squeeze(-1)
        ev64 = compute_errors_l1ssim(level["rgb"].double(), gt.double().unsqueeze(-2)).squeeze(-1)
        e32 = ev32.amin(-1)
        D = (e32.double() - ev64.amin(-1)).abs().max().item()
        comp[f"{name}_bound"] = bound_map(name, e32, upper, D, seed=SEEDS[name] + 1).numpy()
        comp[f"{name}_D"] = np.array([D])
        arrays.update(comp)
        level, gt, bound = MO.load_inputs(comp, name)
        print(name, "D", D, "| lower population", [(e32[s][~upper[s]].min().item(), e32[s][~upper[s]].max().item()) for s in range(n)],
              "| upper from", [e32[s][upper[s]].min().item() for s in range(n)])
        if nv > 1:      # every pixel's two smallest e_v are more than 1e-6 apart (a tie goes to the first view in every l1+ssim kernel)
            two = ev32.sort(-1).values[..., :2]
            assert ((two[..., 1] - two[..., 0]) > 1e-6).all(), "two views (nearly) tie under l1+ssim"
        wsum, std = MO.PO.diverse_stats(level)
        assert ((std - 0.01).abs() > 1e-4).all() and ((wsum - 0.9).abs() > 1e-4).all(), "a (ray, view) sits on a comparison of the diverse rule"
        for cname in MO.CONFIGS:
            cfg, am = MO.config_of(cname), MO.automasked(cname)
            b = bound if am else None
            gt_in = torch.cat((gt, bound.unsqueeze(-1)), dim=-1) if am else gt

            def ref_fn(lv, g_):
                if am:      # the reference renders the map's channel too and cuts it off first thing
                    lv = dict(lv, rgb=torch.cat((lv["rgb"], torch.zeros_like(lv["rgb"][..., :1])), dim=-1))
                return ref.ReconstructionLoss(dict(cfg), am)(dict(coarse=[lv], fine=[dict(lv)], rgb_gt=g_))
            want = run(ref_fn, level, gt_in)
            got = run(lambda lv, g_: MO.reconstruction_loss(lv, gt, cfg, bound=b), level, gt)
            assert abs(want[0].item() - got[0].item()) <= 1e-6, (name, cname, want[0], got[0])
            for x, y in ((want[2], got[2]), (want[3], got[3])):
                assert (x - y).abs().max().item() <= 1e-5 * x.abs().max().item(), (name, cname)
            o = got[1]
            lv64, gt64, b64 = MO.to_double(level, gt, b)
            thr64 = MO.reconstruction_loss(lv64, gt64, cfg, bound=b64)[1]["thresholds"]
            e, thr = o["e"].reshape(n, -1), o["thresholds"]
            gaps = []
            for s in range(n):
                srt = e[s].sort().values
                assert srt[rank] == thr[s]
                above = e[s][e[s] > thr[s]]
                gaps.append((above.min() - thr[s]).item())
                assert gaps[-1] >= 20 * D, (name, cname, s, gaps[-1], D)
                if name == "p8" and s == 0:
                    assert srt[rank + 1] == srt[rank] and int((e[s] <= thr[s]).sum()) == rank + 2, "the <= tie is not there"
            frac = 1 - o["keep"].reshape(n, -1).mean(-1)
            if name == "odd" and cfg["invalid_policy"] != "none":
                assert frac[-1] > 0.5 and thr[-1] == 0 and (thr[:-1] > 0).all() and (frac[:-1] < 0.5).all()
            else:
                assert (frac < 0.5).all() and (thr > 0).all()
            assert (frac > 0).all() == (cfg["invalid_policy"] != "none")
            if am:
                e0 = MO.errors(level, gt)[0].squeeze(-1)
                share = (e0 > bound).float().mean().item()
                assert 0.2 <= share <= 0.8 and ((e0 - bound).abs() >= 20 * D).all(), (name, share)
            for m, cfgs in MUTANT_CONFIGS.items():
                if cname in cfgs and moved(got, run(lambda lv, g_: MO.reconstruction_loss(lv, gt, cfg, bound=b, mutant=m), level, gt)):
                    caught[m].add((cname, name))
            key = f"{name}_{cname}"
            arrays.update({f"{key}_loss": want[0].reshape(1).numpy(),
                           f"{key}_loss_dict": np.array([float(want[1][k]) for k in MO.DICT_KEYS], dtype=np.float64),
                           f"{key}_thresholds": thr.numpy(), f"{key}_thresholds64": thr64.numpy(),
                           f"{key}_kept": np.array([o["kept"]], dtype=np.int64),
                           f"{key}_g_rgb": want[2].numpy(), f"{key}_g_depth": want[3].numpy()})
            print(name, cname, "loss", want[0].item(), "thr", thr.tolist(), "kept", o["kept"], "gaps above", gaps, "invalid", frac.tolist())
    for m, cfgs in MUTANT_CONFIGS.items():
        hit = {c for c, _ in caught[m]}
        print("mutant", m, "moves", sorted(caught[m]))
        assert hit == set(cfgs), f"mutant {m} is not caught under {sorted(set(cfgs) - hit)}"
    out = os.path.join(HERE, "loss_ssim_median.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1_000_000


if __name__ == "__main__":
    main()
