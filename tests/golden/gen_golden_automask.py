"""Generates tests/golden/automask.npz FROM THE REAL REFERENCE, on the CPU:

  * the error map of use_automasking: the reference's compute_errors_l1ssim (models/bts/model/loss.py) inside the four lines of
    trainer.py:203-206, restated around it, on the four cases of tests/_automask_oracle.py: MAP_CASES -- frames of 8-bit-quantised smooth
    noise, every view a shifted copy of one scene, plus a band that is identical in all views.  Stored per case: the frames (uint8), the
    fp32 map, the map of the SAME reference code run in fp64, and the fp32 map's largest distance to the fp64 one (the GPU test allows
    the kernel twice that distance to the fp64 map);
  * the reference's ReconstructionLoss(cfg, True) on tensors in reconstruct()'s layout (rendered colours with the dead fourth channel,
    ground truth with the bound as fourth channel) for _automask_oracle.CONFIGS x LAYOUTS.  Stored: the inputs in the compact exact form
    of tests/golden/gen_golden_loss_pixel.py (its construction: in sample 0 a block whose view-0 error is exactly 1 / 8 in every
    channel), one bound map per criterion, the loss, the loss dict and d loss / d rgb, d loss / d depth.

The bound comes from a seeded smooth map, scaled per layout and criterion to the median error so that it binds about half of the
values.  For l1 / l2 it is overwritten, in the left half of patch 0's block, with the dyadic value that ties EXACTLY with view 0's error
(0.125 / 0.015625; the l1 bound of sample 0 stays above 1 / 8 from the block's rows on, so that under median thresholding the block
still holds the sample's median and its rays are kept).  The script ASSERTS on the reference: per configuration and layout the share of compared values the bound binds lies
in [0.2, 0.8]; outside the tie block every |e - thresh| > 1e-4 (no rounding difference between a kernel and the reference flips a
choice); under l1+ssim every pixel's two best views are more than 1e-6 apart; overwriting the rendered fourth channel leaves the
reference's loss unchanged and its gradient is exactly 0; the restatement tests/_automask_oracle.py reproduces the reference; and each
of its mutants moves a stored map, loss or gradient beyond the tests' bars.

    python -B tests/golden/gen_golden_automask.py      (build container only)"""
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
from tests import _automask_oracle as AO
from tests.golden.gen_golden_loss_pixel import compact_inputs

torch.set_num_threads(4)

BAR_LOSS, BAR_GRAD = 1e-5, 1e-4        # the GPU tests' bars: loss absolute, gradients relative to the largest entry
MUTANT_CONFIGS = {"thresh_channel_mean": ("l2", "l1_median", "l2_diverse"), "thresh_after_median": ("l1_median",),
                  "tie_full": ("l2", "l1_median", "l2_diverse")}


def frames_u8(n, v, H, W, seed):
    """smooth noise, one scene per batch element, view k shifted by (k, 2 k) pixels; rows [H / 3, H / 3 + max(H / 6, 1)) are a band that
    is identical in all views"""
    g = torch.Generator().manual_seed(seed)
    pad = 2 * v + 6
    scene = F.avg_pool2d(torch.rand(n, 3, H + pad + 4, W + pad + 4, generator=g), 5, 1, 2)
    scene = (scene - scene.amin()) / (scene.amax() - scene.amin())
    out = torch.empty(n, v, 3, H, W)
    for k in range(v):
        out[:, k] = scene[:, :, 2 + k:2 + k + H, 2 + 2 * k:2 + 2 * k + W]
    b0 = H // 3
    out[:, :, :, b0:b0 + max(H // 6, 1)] = out[:, :1, :, b0:b0 + max(H // 6, 1)]
    return (8 + out * 240).round().to(torch.uint8)


def reference_map(compute_errors_l1ssim, images_ip, ids_loss, n_render):
    """trainer.py:203-206 around the reference's compute_errors_l1ssim"""
    n, v, c, h, w = images_ip.shape
    frames = images_ip.permute(0, 1, 3, 4, 2).reshape(n, v, h, w, 1, c).expand(-1, -1, -1, -1, n_render, -1) * .5
    partners = images_ip[:, ids_loss].permute(0, 3, 4, 1, 2).reshape(n, 1, h, w, n_render, c).expand(-1, v, -1, -1, -1, -1) * .5
    errors = compute_errors_l1ssim(frames, partners).mean(-2).squeeze(-1).unsqueeze(2)
    return torch.cat((images_ip, errors), dim=2)


def run(loss_fn, level, gt4, dead=None):
    """-> loss, parts, d rgb (of the three live channels), d depth; dead: values for the rendered fourth channel (reference only)"""
    lv = dict(level)
    rgb3 = level["rgb"].clone().requires_grad_(True)
    lv["depth"] = level["depth"].clone().requires_grad_(True)
    if dead is not None:
        d = dead.clone().requires_grad_(True)
        lv["rgb"] = torch.cat((rgb3, d), dim=-1)
        # (rgb_samps stays at three channels: weight_guided_diverse would average the reference's std over the map's channel too)
    else:
        lv["rgb"] = rgb3
    loss, parts = loss_fn(lv, gt4)
    g_rgb, g_depth = torch.autograd.grad(loss, [rgb3, lv["depth"]], retain_graph=dead is not None)
    if dead is not None:
        g_dead, = torch.autograd.grad(loss, [d], allow_unused=True)
        assert g_dead is None or (g_dead == 0).all(), "the rendered fourth channel receives a gradient"
    return loss.detach(), parts, g_rgb, g_depth


def moved(a, b):
    return (abs(a[0].item() - b[0].item()) > BAR_LOSS or (a[2] - b[2]).abs().max().item() > BAR_GRAD * a[2].abs().max().item())


def bound_map(level, gt, cfg, layout, ckey, seed, tie):
    """the per-ray bound (n, pc, h, w) of one layout and criterion"""
    n, pc, h, w = level["depth"].shape
    g = torch.Generator().manual_seed(seed)
    u = F.avg_pool2d(torch.rand(n * pc, 1, h + 4, w + 4, generator=g), 3, 1, 1)[:, 0, 2:-2, 2:-2].reshape(n, pc, h, w)
    u = (u - u.amin()) / (u.amax() - u.amin())
    e = AO.errors_before_bound(level, gt, cfg)
    t = (e.median() * (0.25 + 1.5 * u) * 2 ** 20).round() / 2 ** 20
    a0 = (h * 35) // 100
    if ckey == "l1":
        # l1 runs with median thresholding: from the block's first row on, sample 0's bounds stay above the block's error 1 / 8, so that
        # the block still holds the sample's median (compact_inputs' construction) and the tied rays are among the kept ones
        t[0, :, a0:] = torch.maximum(t[0, :, a0:], torch.tensor(0.125 + 1.0 / 512))
    for _ in range(64):          # away from every compared value: a kernel's rounding must not flip a choice
        near = ((e - t.unsqueeze(-1)).abs() <= 2e-4).any(-1)
        if not near.any():
            break
        t = torch.where(near, t + 1.0 / 1024, t)
    block = torch.zeros(n, pc, h, w, dtype=torch.bool)
    if tie is not None:
        a, b = (h * 35) // 100, (h * 65 + 99) // 100        # compact_inputs' rows of sample 0 with view 0's exact error 1 / 8
        block[0, 0, a:b, : w // 2] = True
        t[block] = tie
        assert (e[block] == tie).all(), "the constructed block does not tie"
    assert ((e - t.unsqueeze(-1)).abs()[~block] > 1e-4).all(), (layout, ckey)
    return t.float().contiguous(), block


def main():
    ref = load_reference()
    from models.bts.model.loss import compute_errors_l1ssim
    arrays = {}
    # ---- the map
    caught = {m: set() for m in AO.MAP_MUTANTS}
    for case, (n, v, H, W, ids) in AO.MAP_CASES.items():
        u8 = frames_u8(n, v, H, W, seed=1700 + H)
        arrays[f"map_{case}_u8"] = u8.numpy()
        arrays[f"map_{case}_ids"] = np.array(ids, dtype=np.int32)
        x = AO.map_frames(arrays, case)
        ref32 = reference_map(compute_errors_l1ssim, x, ids, len(ids))
        ref64 = reference_map(compute_errors_l1ssim, x.double(), ids, len(ids))
        assert torch.equal(ref32[:, :, :3], x) and ref32.shape == (n, v, 4, H, W)
        m32, m64 = ref32[:, :, 3], ref64[:, :, 3]
        dist = (m32.double() - m64).abs().max().item()
        got = AO.error_map(x, ids)
        assert (got[:, :, 0] - m32).abs().max().item() <= 1e-6 and torch.equal(AO.images4(x, ids)[:, :, :3], x), case
        assert (AO.error_map(x.double(), ids)[:, :, 0] - m64).abs().max().item() <= 1e-12, case
        for m in AO.MAP_MUTANTS:
            if (AO.error_map(x, ids, mutant=m)[:, :, 0].double() - m64).abs().max().item() > 2 * dist:
                caught[m].add(case)
        arrays.update({f"map_{case}_ref32": m32.numpy(), f"map_{case}_ref64": m64.numpy(), f"map_{case}_dist": np.array([dist])})
        print("map", case, (n, v, H, W), ids, "fp32 reference to fp64:", dist, "-> bar", 2 * dist, "| map range", m64.min().item(), m64.max().item())
    for m in AO.MAP_MUTANTS:
        print("map mutant", m, "moves", sorted(caught[m]))
        assert caught[m], f"map mutant {m} is not caught"
    # ---- the loss
    caught = {m: set() for m in AO.LOSS_MUTANTS}
    for layout, (n, pc, h, w, nv, K) in AO.LAYOUTS.items():
        for seed in range(1800 + h + w, 1800 + h + w + 1000, 100):      # the first seed without a near-tie of two views under l1+ssim
            comp = compact_inputs(f"am_{layout}", n, pc, h, w, nv, K, seed=seed)
            level, gt = AO.load_inputs(comp, layout)
            two = AO.OL.errors_l1ssim(level["rgb"], gt.unsqueeze(-2)).squeeze(-1).sort(-1).values[..., :2]
            if ((two[..., 1] - two[..., 0]) > 1e-6).all():
                break
        arrays.update(comp)
        assert ((two[..., 1] - two[..., 0]) > 1e-6).all(), "two views (nearly) tie under l1+ssim"
        print(layout, "smallest gap between the two best views under l1+ssim", (two[..., 1] - two[..., 0]).min().item())
        blocks = {}
        for i, ckey in enumerate(("ssim", "l1", "l2")):
            cfg = dict(criterion="l1+ssim" if ckey == "ssim" else ckey)
            t, blocks[ckey] = bound_map(level, gt, cfg, layout, ckey, seed=1900 + 10 * h + i, tie=AO.TIE.get(ckey))
            arrays[f"am_{layout}_thresh_{ckey}"] = t.numpy()
        arrays[f"am_{layout}_tie_block"] = blocks["l1"].numpy()
        dead = torch.rand(level["rgb"].shape[:-1] + (1,), generator=torch.Generator().manual_seed(7))
        for cname in AO.CONFIGS:
            cfg = AO.config_of(cname)
            gt4 = torch.cat((gt, AO.load_thresh(arrays, layout, cname).unsqueeze(-1)), dim=-1)

            def ref_fn(lv, g):
                return ref.ReconstructionLoss(dict(cfg), True)(dict(coarse=[lv], fine=[dict(lv)], rgb_gt=g))
            want = run(ref_fn, level, gt4, dead=dead)
            again = run(ref_fn, level, gt4, dead=dead * 3 - 1)
            assert want[0].item() == again[0].item() and torch.equal(want[2], again[2]), "the rendered fourth channel changes the loss"
            got = run(lambda lv, g: AO.reconstruction_loss(lv, g, cfg), level, gt4)
            assert abs(want[0].item() - got[0].item()) <= 1e-6, (layout, cname, want[0], got[0])
            for x, y in ((want[2], got[2]), (want[3], got[3])):
                assert (x - y).abs().max().item() <= 1e-5 * x.abs().max().item(), (layout, cname)
            share = got[1]["bound"]
            assert 0.2 <= share <= 0.8, (layout, cname, share)
            for m, cfgs in MUTANT_CONFIGS.items():
                if cname in cfgs and moved(want, run(lambda lv, g: AO.reconstruction_loss(lv, g, cfg, mutant=m), level, gt4)):
                    caught[m].add((cname, layout))
            key = f"am_{layout}_{cname}"
            arrays.update({f"{key}_loss": want[0].reshape(1).numpy(),
                           f"{key}_loss_dict": np.array([float(want[1][k]) for k in AO.DICT_KEYS], dtype=np.float64),
                           f"{key}_g_rgb": want[2].numpy(), f"{key}_g_depth": want[3].numpy()})
            print(layout, cname, "loss", want[0].item(), "bound share", share, "kept", got[1]["kept"])
    for m, cfgs in MUTANT_CONFIGS.items():
        hit = {c for c, _ in caught[m]}
        print("loss mutant", m, "moves", sorted(caught[m]))
        assert hit == set(cfgs), f"mutant {m} is not caught under {sorted(set(cfgs) - hit)}"
    out = os.path.join(HERE, "automask.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1_000_000


if __name__ == "__main__":
    main()
