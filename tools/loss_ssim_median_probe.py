"""ms per call of criterion l1+ssim WITH median thresholding (`native_ssim_median: true`: bts_photometric_loss_median, the median variant
of csrc/bts_loss_tiled.hip's passes) on one GPU, in ONE process, each shape against

  shipped   the shipped entry WITHOUT median thresholding on the same inputs (8 x 8 patches: the wave kernel bts_photometric_loss, the
            frame: bts_photometric_loss_tiled) -- the parent's code, so the difference is the cost of the option
  eager     an eager torch restatement of the reference's sequence for l1+ssim + median (models/bts/model/loss.py:83-293 with
            lambda_edge_aware_smoothness = 0.01; without its .item() synchronisations, which only favours it)

  train_p8  16 x 4096 rays in 8 x 8 patches, nv = 4, K = 64, weight_guided, forward + gradients with respect to rgb and depth
  val       one 192 x 640 validation frame (n = 1, v = 2 frames as ImageRaySampler.reconstruct lays them out, nv = 1, K = 64), strict,
            forward only (under no_grad)

with HIP events over --iters iterations after --warmup warm-ups (mean of the timed window).  The sides of every comparison are
alternated in four blocks, so that a drifting clock meets all of them; the blocks are printed, `separated` says whether the slowest
block of the faster side is faster than the fastest block of the slower side.  Prints ONE JSON line and, with --out, writes the same
numbers as text.

    python tools/loss_ssim_median_probe.py [--out profiles/r18a/loss_ssim_median.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from tools.loss_pixel_probe import K, LAMBDA_EAS, _eas, inputs, mean_ms  # noqa: E402

_WINDOW = torch.tensor([[0.0947, 0.1183, 0.0947], [0.1183, 0.1478, 0.1183], [0.0947, 0.1183, 0.0947]])


def _ssim(x, y):
    """layers.py:123-150 with pad_reflection=False, gaussian_average=True, comp_mode=True"""
    k = _WINDOW.to(x.device).repeat(x.shape[1], 1, 1, 1)
    gauss = lambda t: F.conv2d(t, k, padding=0, groups=t.shape[1])
    x, y = F.pad(x, (1, 1, 1, 1)), F.pad(y, (1, 1, 1, 1))
    mu_x, mu_y = gauss(x), gauss(y)
    sigma_x, sigma_y, sigma_xy = gauss(x ** 2) - mu_x ** 2, gauss(y ** 2) - mu_y ** 2, gauss(x * y) - mu_x * mu_y
    n = (2 * mu_x * mu_y + 0.01 ** 2) * (2 * sigma_xy + 0.03 ** 2)
    d = (mu_x ** 2 + mu_y ** 2 + 0.01 ** 2) * (sigma_x + sigma_y + 0.03 ** 2)
    return torch.clamp(1 - n / d, 0, 1) / 2


def _errors(img0, img1):
    """loss.py:10-18"""
    n, pc, h, w, nv, c = img0.shape
    a = img0.permute(0, 1, 4, 5, 2, 3).reshape(-1, c, h, w)
    b = img1.expand(img0.shape).permute(0, 1, 4, 5, 2, 3).reshape(-1, c, h, w)
    e = .85 * torch.mean(_ssim(a, b), dim=1) + .15 * torch.mean(torch.abs(a - b), dim=1)
    return e.view(n, pc, nv, h, w).permute(0, 1, 3, 4, 2).unsqueeze(-1)


def eager_loss(level, rgb_gt, policy):
    inv, wts = level["invalid"], level["weights"]
    if policy == "strict":
        invalid = torch.all(torch.any(inv > .5, dim=-2), dim=-1).unsqueeze(-1)
    else:
        invalid = torch.all((inv.to(torch.float32) * wts.unsqueeze(-1)).sum(-2) > .9, dim=-1, keepdim=True)
    keep = 1 - invalid.to(torch.float32)
    gt = rgb_gt.unsqueeze(-2)
    b = level["rgb"].shape[0]
    terms = []
    for _ in range(2):        # the reference evaluates the aliased fine dict again (:171-184)
        e = _errors(level["rgb"], gt).amin(-2) * keep
        thr = torch.median(e.view(b, -1), dim=-1)[0].view(-1, 1, 1, 1, 1)
        terms.append(e[e <= thr].mean())
    eas = _eas(gt, level["depth"])
    eas = (eas * (1 - torch.ceil(F.interpolate(invalid.squeeze(-1).to(torch.float32), size=level["depth"].shape[-2:])))).mean()
    return terms[0] + terms[1] + eas * LAMBDA_EAS


def blocks(fns, iters, warmup):
    """fns: {side: callable}, alternated in four blocks -> per side the mean and its blocks, and the ratios to `median`"""
    t = {k: [] for k in fns}
    for _ in range(4):
        for k, fn in fns.items():
            t[k].append(mean_ms(fn, max(iters // 4, 1), warmup // 4 + 1))
    out = {k: round(sum(v) / 4, 4) for k, v in t.items()}
    out.update({f"{k}_blocks": [round(x, 4) for x in v] for k, v in t.items()})
    for k in fns:
        if k != "median":
            out[f"{k}_over_median"] = round(out[k] / out["median"], 2)
            lo, hi = (t["median"], t[k]) if out["median"] <= out[k] else (t[k], t["median"])
            out[f"{k}_separated"] = max(lo) < min(hi)
    return out


CASES = (("train_p8", (16, 64, 8, 8, 4), True, "weight_guided"), ("val", (1, 2, 192, 640, 1), False, "strict"))


def run(iters, warmup):
    out = dict(metric="ms_per_call", K=K, iters=iters, warmup=warmup)
    for tag, shape, grad, policy in CASES:
        conf = dict(criterion="l1+ssim", invalid_policy=policy, lambda_edge_aware_smoothness=LAMBDA_EAS)
        crit_med = bts.ReconstructionLoss(dict(conf, median_thresholding=True, native_ssim_median=True))
        crit_shipped = bts.ReconstructionLoss(conf)
        level, gt = inputs(*shape, seed=13, grad=grad, samps=False)
        data = dict(coarse=[level], fine=[dict(level)], rgb_gt=gt)

        def through(f):
            def call():
                if grad:
                    torch.autograd.grad(f(), [level["rgb"], level["depth"]])
                else:
                    with torch.no_grad():
                        f()
            return call

        with torch.no_grad():
            out[f"{tag}_loss_median_vs_eager"] = [crit_med(data)[0].item(), eager_loss(level, gt, policy).item()]
        out[tag] = blocks(dict(median=through(lambda: crit_med(data)[0]), shipped=through(lambda: crit_shipped(data)[0]),
                               eager=through(lambda: eager_loss(level, gt, policy))), iters, warmup)
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
        sys.exit("loss_ssim_median_probe: no GPU; nothing is measured without one")
    res = run(args.iters, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("l1+ssim with median thresholding (native_ssim_median: bts_photometric_loss_median) against the shipped entry without median and "
                    f"an eager torch restatement, ms per call (tools/loss_ssim_median_probe.py; HIP events, mean over {res['iters']} iterations "
                    f"after {res['warmup']} warm-ups, alternated in four blocks)\n")
            for k, v in res.items():
                f.write(f"{k:36s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
