"""ms per call of the per-pixel criteria of ReconstructionLoss (`native_pixel_loss: true`: bts_pixel_loss, csrc/bts_loss_pixel.hip) against
an eager torch restatement of the reference's loss sequence (models/bts/model/loss.py:83-293 for the same setting, with
lambda_edge_aware_smoothness = 0.01; without its nine .item() synchronisations, which only favours it) on the same GPU, in ONE process:

  train_p8_*        16 x 4096 rays in 8 x 8 patches, nv = 4, K = 64, forward + gradients with respect to rgb and depth, for
                    l2 (strict), l2 + median (weight_guided), l2 + weight_guided_diverse
  val_*             one 192 x 640 validation frame (n = 1, v = 2 frames as ImageRaySampler.reconstruct lays them out, nv = 1, K = 64),
                    forward only (under no_grad), for l2 (strict) and l1 + median (strict)

with HIP events over --iters iterations after --warmup warm-ups (mean of the timed window).  The two sides of every comparison are
alternated in four blocks, so that a drifting clock meets both; `separated` says whether the slowest library block is faster than the
fastest eager block.  Prints ONE JSON line and, with --out, writes the same numbers as text.

    python tools/loss_pixel_probe.py [--out profiles/r15a/loss_pixel.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402

LAMBDA_EAS = 0.01
K = 64


def mean_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


# ---- the reference's op sequence, restated in eager torch (loss.py:21-40, 83-293)
def _eas(gt_img, depth):
    n, pc, h, w = depth.shape
    gt = gt_img.permute(0, 1, 4, 5, 2, 3).reshape(-1, 3, h, w)
    d = 1 / depth.reshape(-1, 1, h, w).clamp(1e-3, 80)
    d = d / torch.mean(d, dim=[2, 3], keepdim=True)
    d_dx, d_dy = torch.abs(d[:, :, :, :-1] - d[:, :, :, 1:]), torch.abs(d[:, :, :-1, :] - d[:, :, 1:, :])
    i_dx = torch.mean(torch.abs(gt[:, :, :, :-1] - gt[:, :, :, 1:]), 1, keepdim=True)
    i_dy = torch.mean(torch.abs(gt[:, :, :-1, :] - gt[:, :, 1:, :]), 1, keepdim=True)
    return (F.pad(d_dx * torch.exp(-i_dx), (0, 1)) + F.pad(d_dy * torch.exp(-i_dy), (0, 0, 0, 1))).view(n, pc, h, w)


def eager_loss(level, rgb_gt, conf):
    inv, wts = level["invalid"], level["weights"]
    policy = conf["invalid_policy"]
    if policy == "strict":
        invalid = torch.all(torch.any(inv > .5, dim=-2), dim=-1).unsqueeze(-1)
    elif policy == "weight_guided":
        invalid = torch.all((inv.to(torch.float32) * wts.unsqueeze(-1)).sum(-2) > .9, dim=-1, keepdim=True)
    else:
        std = torch.std(level["rgb_samps"], dim=-3).mean(-1)
        invalid = torch.all(((inv.to(torch.float32) * wts.unsqueeze(-1)).sum(-2) > .9) | (std < 0.01), dim=-1, keepdim=True)
    keep = 1 - invalid.to(torch.float32)
    gt = rgb_gt.unsqueeze(-2)
    crit = torch.nn.MSELoss(reduction="none") if conf["criterion"] == "l2" else torch.nn.L1Loss(reduction="none")
    b = level["rgb"].shape[0]
    terms = []
    for _ in range(2):        # the reference evaluates the aliased fine dict again (:171-184)
        e = crit(level["rgb"], gt.expand(level["rgb"].shape)).amin(-2) * keep
        if conf.get("median_thresholding"):
            thr = torch.median(e.view(b, -1), dim=-1)[0].view(-1, 1, 1, 1, 1)
            e = e[e <= thr]
        terms.append(e.mean())
    eas = _eas(gt, level["depth"])
    eas = (eas * (1 - torch.ceil(F.interpolate(invalid.squeeze(-1).to(torch.float32), size=level["depth"].shape[-2:])))).mean()
    return terms[0] + terms[1] + eas * LAMBDA_EAS


def inputs(n, pc, h, w, nv, seed, grad, samps):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = dict(device="cuda", generator=g)
    gt = F.avg_pool2d(torch.rand(n * pc, 3, h + 4, w + 4, **r), 3, 1, 1)[:, :, 2:-2, 2:-2]
    gt = gt.reshape(n, pc, 3, h, w).permute(0, 1, 3, 4, 2).contiguous()
    rgb = (gt.unsqueeze(-2) + 0.15 * torch.randn(n, pc, h, w, nv, 3, **r)).clamp(0, 1)
    depth = torch.rand(n, pc, h, w, **r) * 100 + 0.5
    wts = torch.rand(n, pc, h, w, K, **r)
    wts = wts / wts.sum(-1, keepdim=True)
    # a fifth of the (ray, view) pairs have invalid samples at all (strict would otherwise call every ray invalid and the loss be 0)
    inv = ((torch.rand(n, pc, h, w, K, nv, **r) < 0.3) & (torch.rand(n, pc, h, w, 1, nv, **r) < 0.2)).float()
    inv[:, :, 0] = 1.0
    level = dict(rgb=rgb.requires_grad_(grad), depth=depth.requires_grad_(grad), weights=wts, invalid=inv)
    if samps:
        level["rgb_samps"] = torch.rand(n, pc, h, w, K, nv, 3, **r)
    return level, gt


def blocks(fn_lib, fn_eager, iters, warmup):
    t_lib, t_eager = [], []
    for _ in range(4):
        t_lib.append(mean_ms(fn_lib, max(iters // 4, 1), warmup // 4 + 1))
        t_eager.append(mean_ms(fn_eager, max(iters // 4, 1), warmup // 4 + 1))
    lib, eager = sum(t_lib) / 4, sum(t_eager) / 4
    return dict(library=round(lib, 4), eager=round(eager, 4), ratio=round(eager / lib, 2), separated=max(t_lib) < min(t_eager),
                library_blocks=[round(t, 4) for t in t_lib], eager_blocks=[round(t, 4) for t in t_eager])


CASES = (("train_p8_l2", (16, 64, 8, 8, 4), True, dict(criterion="l2", invalid_policy="strict")),
         ("train_p8_l2_median", (16, 64, 8, 8, 4), True, dict(criterion="l2", invalid_policy="weight_guided", median_thresholding=True)),
         ("train_p8_l2_diverse", (16, 64, 8, 8, 4), True, dict(criterion="l2", invalid_policy="weight_guided_diverse")),
         ("val_l2", (1, 2, 192, 640, 1), False, dict(criterion="l2", invalid_policy="strict")),
         ("val_l1_median", (1, 2, 192, 640, 1), False, dict(criterion="l1", invalid_policy="strict", median_thresholding=True)))


def run(iters, warmup):
    out = dict(metric="ms_per_call", K=K, iters=iters, warmup=warmup)
    for tag, shape, grad, conf in CASES:
        crit = bts.ReconstructionLoss(dict(conf, lambda_edge_aware_smoothness=LAMBDA_EAS, native_pixel_loss=True))
        level, gt = inputs(*shape, seed=13, grad=grad, samps=conf["invalid_policy"] == "weight_guided_diverse")
        data = dict(coarse=[level], fine=[dict(level)], rgb_gt=gt)

        def lib():
            if grad:
                torch.autograd.grad(crit(data)[0], [level["rgb"], level["depth"]])
            else:
                with torch.no_grad():
                    crit(data)

        def eager():
            if grad:
                torch.autograd.grad(eager_loss(level, gt, conf), [level["rgb"], level["depth"]])
            else:
                with torch.no_grad():
                    eager_loss(level, gt, conf)

        with torch.no_grad():
            out[f"{tag}_loss_library_vs_eager"] = [crit(data)[0].item(), eager_loss(level, gt, conf).item()]
        out[tag] = blocks(lib, eager, iters, warmup)
        del level, gt, data
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_pixel_probe: no GPU; nothing is measured without one")
    res = run(args.iters, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("Per-pixel criteria of ReconstructionLoss (native_pixel_loss: l1 / l2, median thresholding, weight_guided_diverse), ms per call "
                    f"(tools/loss_pixel_probe.py; HIP events, mean over {res['iters']} iterations after {res['warmup']} warm-ups, alternated in "
                    "four blocks)\n")
            for k, v in res.items():
                f.write(f"{k:36s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
