"""ms per call of ReconstructionLoss with its optional regularisers on (alpha_reg, surfaceness, ray entropy, depth_reg +
depth_smoothness) on one GPU, in ONE process, each shape on

  native   `native_regularisers: true`: bts_loss_regularisers (csrc/bts_loss_reg.hip), one call per scale
  torch    the same tree without the key: the torch composition of loss.py's _call -- the parent's code

  train_p8_alpha_ray   16 x 4096 rays in 8 x 8 patches, nv = 4, K = 64, weight_guided, alpha_reg (ray) alone, forward + gradients with
                       respect to rgb, depth and alphas
  train_p8_all         the same with every regulariser on
  val_all              one 192 x 640 validation frame (n = 1, v = 2 frames as ImageRaySampler.reconstruct lays them out, nv = 1, K = 64),
                       strict, every regulariser on, forward only (under no_grad)

with HIP events over --iters iterations after --warmup warm-ups (mean of the timed window).  Both sides are alternated in four blocks,
so that a drifting clock meets both; the blocks are printed, `separated` says whether the slowest block of the faster side is faster
than the fastest block of the slower side.  Both sides must return the same loss (1e-5).  The photometric term (l1+ssim with
lambda_edge_aware_smoothness = 0.01: the shipped HIP pass) is part of both sides; `photometric` times it alone (no regulariser: the
linear-matrix path) for scale.  Prints ONE JSON line and, with --out, writes the same numbers as text.

    python tools/loss_reg_probe.py [--out profiles/r19a/loss_reg.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from tools.loss_pixel_probe import K, LAMBDA_EAS, inputs, mean_ms  # noqa: E402

ALL = dict(lambda_alpha_reg=0.05, lambda_surfaceness_reg=0.1, lambda_entropy=0.02, lambda_depth_reg=0.03, lambda_depth_smoothness=0.02)
CASES = (("train_p8_alpha_ray", (16, 64, 8, 8, 4), True, "weight_guided", dict(lambda_alpha_reg=0.05, alpha_reg_reduction="ray")),
         ("train_p8_all", (16, 64, 8, 8, 4), True, "weight_guided", dict(ALL, alpha_reg_reduction="ray")),
         ("val_all", (1, 2, 192, 640, 1), False, "strict", dict(ALL, alpha_reg_reduction="ray")))


def blocks(fns, iters, warmup):
    """fns: {side: callable}, alternated in four blocks -> per side the mean and its blocks; torch over native and whether they separate"""
    t = {k: [] for k in fns}
    for _ in range(4):
        for k, fn in fns.items():
            t[k].append(mean_ms(fn, max(iters // 4, 1), warmup // 4 + 1))
    out = {k: round(sum(v) / 4, 4) for k, v in t.items()}
    out.update({f"{k}_blocks": [round(x, 4) for x in v] for k, v in t.items()})
    out["torch_over_native"] = round(out["torch"] / out["native"], 2)
    lo, hi = (t["native"], t["torch"]) if out["native"] <= out["torch"] else (t["torch"], t["native"])
    out["separated"] = max(lo) < min(hi)
    return out


def run(iters, warmup):
    out = dict(metric="ms_per_call", K=K, iters=iters, warmup=warmup)
    for tag, shape, grad, policy, reg in CASES:
        conf = dict(criterion="l1+ssim", invalid_policy=policy, lambda_edge_aware_smoothness=LAMBDA_EAS)
        crits = dict(native=bts.ReconstructionLoss(dict(conf, **reg, native_regularisers=True)), torch=bts.ReconstructionLoss(dict(conf, **reg)),
                     photometric=bts.ReconstructionLoss(conf))
        level, gt = inputs(*shape, seed=13, grad=grad, samps=False)
        n, pc, h, w = level["depth"].shape
        g = torch.Generator(device="cuda").manual_seed(17)
        level["depth"] = (2 + 0.5 * torch.rand(n, pc, h, w, device="cuda", generator=g)).requires_grad_(grad)
        level["alphas"] = (torch.rand(n, pc, h, w, K, device="cuda", generator=g) * 0.25).requires_grad_(grad)
        data = dict(coarse=[level], fine=[dict(level)], rgb_gt=gt)
        wrt = [level["rgb"], level["depth"], level["alphas"]]

        def through(crit, leaves):
            def call():
                if grad:
                    torch.autograd.grad(crit(data)[0], leaves)
                else:
                    with torch.no_grad():
                        crit(data)
            return call

        with torch.no_grad():
            a, b = crits["native"](data)[0].item(), crits["torch"](data)[0].item()
        out[f"{tag}_loss_native_vs_torch"] = [a, b]
        assert abs(a - b) <= 1e-5, (tag, a, b)
        out[tag] = blocks(dict(native=through(crits["native"], wrt), torch=through(crits["torch"], wrt),
                               photometric=through(crits["photometric"], wrt[:2])), iters, warmup)
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
        sys.exit("loss_reg_probe: no GPU; nothing is measured without one")
    res = run(args.iters, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("ReconstructionLoss with its regularisers on: native_regularisers (bts_loss_regularisers) against the torch composition of the "
                    f"same tree without the key, ms per call (tools/loss_reg_probe.py; HIP events, mean over {res['iters']} iterations after "
                    f"{res['warmup']} warm-ups, alternated in four blocks)\n")
            for k, v in res.items():
                f.write(f"{k:36s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
