"""ms per call of the trainer's visualisation panels on one GPU, in ONE process, at the KITTI-360 visualisation frame (v = 8 rendered
frames of 192 x 640, K = 64, nv = 1, one depth scale; T = 6 of them are shown), on

  native   behindthescenes_amd.train_vis.vis_panels: ONE bts_train_vis call (csrc/bts_train_vis.hip, two launches), nothing synchronises
  torch    an eager torch restatement of the reference's sequence (models/bts/trainer.py:436-484) on the same GPU, INCLUDING its colour
           mapping: seven maps pulled to the host, matplotlib's colour map in float64, the colours sent back (utils/plotting.py:41-46).
           (``alphas + 1e-5`` is out of place here, one pass like the reference's in-place add: in place it would drift over the loop.)

with HIP events over --iters iterations after --warmup warm-ups (mean of the timed window).  Both sides are alternated in four blocks,
so that a drifting clock meets both; the blocks are printed, `separated` says whether the slowest block of the faster side is faster
than the fastest block of the slower side.  `native_gbs` is the compulsory traffic over native's time: T h w K (1 + nv) 4 bytes of
alphas and invalid, plus the small maps (images, colours and depths read, the panels written, the three profile rows read again).
Both sides' scalar fields are compared once (the largest distance is printed).  Prints ONE JSON line and, with --out, writes the
same numbers as text.

    python tools/train_vis_probe.py [--out profiles/r25a/train_vis.txt]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from behindthescenes_amd import train_vis as TV  # noqa: E402
from tools.loss_pixel_probe import mean_ms  # noqa: E402

V, H, W, K, NV, S = 8, 192, 640, 64, 1, 1
Z_NEAR, Z_FAR = 3.0, 80.0


def inputs():
    g = torch.Generator(device="cuda").manual_seed(25)
    r = lambda *s: torch.rand(*s, device="cuda", generator=g)         # noqa: E731
    part = dict(alphas=r(1, V, H, W, K) ** 2, invalid=(r(1, V, H, W, K, NV) < 0.3).float())
    fine = [dict(rgb=r(1, V, H, W, NV, 3), depth=Z_NEAR + (Z_FAR - Z_NEAR) * r(1, V, H, W)) for _ in range(S)]
    return dict(imgs=[r(1, 3, H, W) * 2 - 1 for _ in range(V)], coarse=[part], fine=fine,
                z_near=torch.tensor(Z_NEAR, device="cuda"), z_far=torch.tensor(Z_FAR, device="cuda"))


def eager(data, cmap, fields=None):
    """the reference's sequence; ``fields``: a dict that receives the scalar fields"""
    def color_tensor(x, name):
        if fields is not None:
            fields[name] = x
        return torch.tensor(cmap(x.cpu().numpy()), device=x.device)[..., :3]
    images = torch.stack(data["imgs"], dim=1).detach()[0]
    recon = data["fine"][0]["rgb"].detach()[0]
    depths = [f["depth"].detach()[0] for f in data["fine"]]
    profile = data["coarse"][0]["alphas"].detach()[0]
    alphas = data["coarse"][0]["alphas"].detach()[0]
    invalids = data["coarse"][0]["invalid"].detach()[0]
    z_near, z_far = data["z_near"], data["z_far"]
    T = min(images.shape[0], 6)
    _, c, h, w = images.shape
    images = images[:T] * .5 + .5
    recon = recon.view(recon.shape[0], h, w, -1, c)[:T].mean(dim=-2).permute(0, 3, 1, 2)
    out = dict(input_im=images, recon_im=recon)
    out["recon_mse"] = color_tensor((((images - recon) ** 2) / 2).mean(dim=1).clamp(0, 1), "f_mse").permute(0, 3, 1, 2)
    for s, d in enumerate(depths):
        d = (1 / d[:T] - 1 / z_far) / (1 / z_near - 1 / z_far)
        out[f"recon_depth_{s}"] = color_tensor(d.squeeze(1).clamp(0, 1), f"f_depth_{s}").permute(0, 3, 1, 2)
    profile = profile[:T][:, [h // 4, h // 2, 3 * h // 4], :, :].view(T * 3, w, -1).permute(0, 2, 1)
    out["depth_profile"] = color_tensor(profile.clamp_min(0) / profile.max(), "f_profile").permute(0, 3, 1, 2)
    alphas = alphas[:T] + 1e-5
    p = alphas / alphas.sum(dim=-1, keepdim=True)
    out["ray_entropy"] = color_tensor(-(p * torch.log(p)).sum(-1) / math.log2(alphas.shape[-1]), "f_entropy").permute(0, 3, 1, 2)
    out["alpha_sum"] = color_tensor((alphas.sum(dim=-1) / alphas.shape[-1]).clamp(-1), "f_alpha_sum").permute(0, 3, 1, 2)
    out["invalids"] = color_tensor(invalids[:T].mean(-2).mean(-1), "f_invalid").permute(0, 3, 1, 2)
    return out


def run(iters, warmup):
    import matplotlib
    cmap = matplotlib.colormaps["plasma"]
    data = inputs()
    T = min(V, 6)
    f_t = {}
    eager(data, cmap, f_t)
    f_n = TV.vis_panels(data, fields=True)
    gaps = {k: float((f_n[k] - v.reshape(f_n[k].shape)).abs().max()) for k, v in f_t.items()}
    fns = dict(native=lambda: TV.vis_panels(data), torch=lambda: eager(data, cmap))
    t = {k: [] for k in fns}
    for _ in range(4):
        for k, fn in fns.items():
            t[k].append(mean_ms(fn, max(iters // 4, 1), warmup // 4 + 1))
    out = dict(metric="ms_per_call", shape=dict(v=V, T=T, h=H, w=W, K=K, nv=NV, S=S), iters=iters, warmup=warmup, field_gaps=gaps)
    out.update({k: round(sum(v) / 4, 4) for k, v in t.items()})
    out.update({f"{k}_blocks": [round(x, 4) for x in v] for k, v in t.items()})
    out["torch_over_native"] = round(out["torch"] / out["native"], 1)
    lo, hi = (t["native"], t["torch"]) if out["native"] <= out["torch"] else (t["torch"], t["native"])
    out["separated"] = max(lo) < min(hi)
    px = T * H * W
    small = px * 4 * (3 + 3 * NV + S) + px * 4 * (18 + 3 * S) + 3 * T * K * W * 4 * (1 + 3)
    out["compulsory_bytes"] = px * K * (1 + NV) * 4 + small
    out["native_gbs"] = round(out["compulsory_bytes"] / (out["native"] * 1e-3) / 1e9, 1)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_vis_probe: no GPU; nothing is measured without one")
    res = run(args.iters, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("The trainer's visualisation panels: vis_panels (bts_train_vis) against an eager torch restatement of the reference's sequence "
                    f"with its host colour mapping, ms per call (tools/train_vis_probe.py; HIP events, mean over {res['iters']} iterations after "
                    f"{res['warmup']} warm-ups, alternated in four blocks)\n")
            for k, v in res.items():
                f.write(f"{k:20s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
