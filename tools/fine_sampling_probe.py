"""ms per call of what sits between the two renders of a two-pass forward (n_fine > 0) on one GPU, in ONE process, each shape on

  native   `native_fine_sampling: true`: ONE bts_sample_fine call (csrc/bts_sample_fine.hip), the NaN assert a device counter
  torch    the same tree without the key: sample_fine + sample_fine_depth + cat + sort with their two synchronising asserts -- the
           parent's code path

  frame   2 x 192 x 640 = 245 760 rays (n = 1, two frames), Kc = 64, Kf = 32, Kfd = 8, eval mode under no_grad
  train   16 x 4096 rays, the same sample counts, training mode with gradients enabled (forward only is timed)

and per shape five timings: `sampling_*` the sampling alone on the coarse pass' outputs, `forward_*` the two-pass wrapped(...) forward,
`renders` the two render launches alone on fixed samples (forward minus renders = what the sampling adds per frame).  HIP events over
--iters iterations after --warmup warm-ups (mean of the timed window); the sides are alternated in four blocks so that a drifting clock
meets both, the blocks are printed, `separated` says whether the slowest block of the faster side is below the fastest block of the
slower side.  Both sides must produce the same sorted depths where no draw sits on a cdf edge (checked before timing).  Prints ONE JSON
line and, with --out, writes the same numbers as text.

    python tools/fine_sampling_probe.py [--out profiles/r23a/fine_sampling.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from behindthescenes_amd import native, synthetic as S  # noqa: E402
from tools.loss_pixel_probe import mean_ms  # noqa: E402

KC, KF, KFD = 64, 32, 8
CASES = (("frame", 1, 2, None, False), ("train", 16, 2, 4096, True))      # tag, n, frames, rays per sample (None: every pixel), training
H, W = 192, 640


def blocks(fns, iters, warmup):
    t = {k: [] for k in fns}
    for _ in range(4):
        for k, fn in fns.items():
            t[k].append(mean_ms(fn, max(iters // 4, 1), warmup // 4 + 1))
    out = {k: round(sum(v) / 4, 4) for k, v in t.items()}
    out.update({f"{k}_blocks": [round(x, 4) for x in v] for k, v in t.items()})
    return out, t


def separated(lo, hi):
    return max(lo) < min(hi)


def run(iters, warmup):
    out = dict(metric="ms_per_call", Kc=KC, Kf=KF, Kfd=KFD, iters=iters, warmup=warmup)
    for tag, n, v, per_sample, train in CASES:
        scene = S.synthetic_scene(n, v + 1, H, W, 64, seed=5, intrinsics=S.K_KITTI360, smooth=True)
        net = S.build_net(scene, ids_render=(1, 2), train=train)
        rays, _ = bts.ImageRaySampler(3.0, 80.0, H, W).sample(None, scene["poses"][:, :v].cuda(), scene["projs"][:, :v].cuda())
        if per_sample:
            g = torch.Generator().manual_seed(3)
            idx = torch.stack([torch.randperm(rays.shape[1], generator=g)[:per_sample].sort().values for _ in range(n)]).cuda()
            rays = torch.gather(rays, 1, idx.unsqueeze(-1).expand(-1, -1, 8)).contiguous()
        conf = dict(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, depth_std=1.0, lindisp=True, hard_alpha_cap=True)
        side = {k: bts.NeRFRenderer.from_conf(dict(conf, native_fine_sampling=(k == "native"))).cuda().train(train) for k in ("native", "torch")}
        wrapped = {k: r.bind_parallel(net).train(train) for k, r in side.items()}
        flat = rays.reshape(-1, 8)
        B = flat.shape[0]
        grad = torch.enable_grad if train else torch.no_grad
        with torch.no_grad():
            z_c = side["torch"].sample_coarse(flat)
            w_c, _, d_c, *_ = side["torch"].composite(net, flat, z_c, sb=n)
            g = torch.Generator(device="cuda").manual_seed(9)
            u, t = torch.rand(B, KF - KFD, device="cuda", generator=g), torch.rand(B, KF - KFD, device="cuda", generator=g)
            noise = torch.randn(B, KFD, device="cuda", generator=g)
            # the two sides agree (bit for bit on all but the rays with a draw on a cdf edge, where the two cdfs' last bits decide)
            a = native.sample_fine(flat, w_c, z_c, d_c, u, t, noise, 1.0, True)
            r = side["torch"]
            b = torch.sort(torch.cat([z_c, r.sample_fine(flat, w_c, u=u, t=t), r.sample_fine_depth(flat, d_c, noise=noise)], -1), -1).values
            same = (a == b).all(-1).float().mean().item()
            out[f"{tag}_rays_bit_equal"] = round(same, 6)
            assert same > 0.98, same

        def sampling_native():
            native.sample_fine(flat, w_c, z_c, d_c, u, t, noise, 1.0, True, nan_count=side["native"].fine_nan_count)

        def sampling_torch():
            r = side["torch"]
            torch.sort(torch.cat([z_c, r.sample_fine(flat, w_c), r.sample_fine_depth(flat, d_c)], dim=-1), dim=-1)

        def forward(k):
            def call():
                with grad():
                    wrapped[k](rays)
            return call

        def renders():
            with grad():
                r = side["native"]
                r.composite(net, flat, z_c, sb=n, want_alphas=False, want_rgb_samps=False)
                r.composite(net, flat, a, coarse=False, sb=n, want_weights=False, want_alphas=False, want_rgb_samps=False)

        res, t_ = blocks(dict(sampling_native=sampling_native, sampling_torch=sampling_torch, forward_native=forward("native"),
                              forward_torch=forward("torch"), renders=renders), iters, warmup)
        res["rays"] = B
        res["sampling_torch_over_native"] = round(res["sampling_torch"] / res["sampling_native"], 2)
        res["sampling_separated"] = separated(t_["sampling_native"], t_["sampling_torch"])
        res["forward_native_below_torch_separated"] = separated(t_["forward_native"], t_["forward_torch"])
        res["sampling_adds_native"] = round(res["forward_native"] - res["renders"], 4)
        res["sampling_adds_torch"] = round(res["forward_torch"] - res["renders"], 4)
        side["native"].check_fine_samples()
        out[tag] = res
        del net, rays, flat, wrapped, side
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fine_sampling_probe: no GPU; nothing is measured without one")
    res = run(args.iters, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("Two-pass forward (n_fine > 0): native_fine_sampling (one bts_sample_fine call) against the torch composition of the same tree "
                    f"without the key, ms per call (tools/fine_sampling_probe.py; HIP events, mean over {res['iters']} iterations after "
                    f"{res['warmup']} warm-ups, alternated in four blocks)\n")
            for k, v in res.items():
                f.write(f"{k:36s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
