"""ms per call of the patch-colour route (image_processor {type: patch}: 27 channels per render view) at exp_kitti_360.yaml's training
shape -- 16 x 4 096 rays, K = 64, four render views, 192 x 640 frames, (64, 64, 0) -- forward + backward, and forward only on one
192 x 640 frame.  Times, in ONE process,

  patch          the render (bts_render_fwd / _bwd) with native_patch_color: weights -> bts_patch_color_fwd, g_rgb -> bts_patch_color_bwd ->
                 the render's backward
  plain          the same render of the same field without patch colours (three channels per view): patch - plain is what the 27 channels add
  colours        bts_patch_color_fwd (+ _bwd) alone on held weights
  eager          the reference's colour route restated in torch on the same GPU, on the same held weights: grid_sample over the
                 MATERIALISED 27-channel frames for every sample and view, the weighted sum, autograd back to the weights

with HIP events over --iters iterations after --warmup warm-ups, alternated in four blocks so that a drifting clock meets all of them (the
block means are printed).  Both colour routes must return the same rgb within 1e-5, or the probe exits non-zero.  Prints ONE JSON line
and, with --out, writes the same numbers as text.

    python tools/patch_color_probe.py [--out profiles/r27a/patch_color.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from behindthescenes_amd import native, synthetic  # noqa: E402

H, W, C, HD, K, NV = 192, 640, 64, 64, 64, 4
EPS = 1e-3


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


def nets(n):
    scene = synthetic.synthetic_scene(n, NV + 1, H, W, C, seed=9, intrinsics=synthetic.K_KITTI360, yaw_deg=3.0, smooth=True)
    images, projs, poses = (scene[k].cuda() for k in ("images", "projs", "poses"))
    frames = bts.PatchProcessor(3)(images)
    out = []
    for patch in (True, False):
        net = bts.BTSNet(dict(synthetic.field_conf(C, HD, 0, H, W), native_patch_color=True))
        net.encoder = bts.FeatureMapEncoder((H, W), C, num_views=n)
        synthetic.init_mlp_(net.mlp_coarse, seed=7)
        synthetic.set_feature_map(net, scene["feat"])
        net = net.cuda().train()
        net.encode(images, projs, poses, ids_encoder=[0], ids_render=list(range(1, NV + 1)), images_alt=frames if patch else None)
        out.append(net)
    return out[0], out[1], scene, frames[:, 1:].contiguous()


def eager_colours(frames, net, rays, z, weights):
    """models_bts.py:218-234 + nerf.py:298 on materialised frames (n, nv, 27, H, W)"""
    n, nv = frames.shape[:2]
    pts = (rays[:, None, :3] + z.unsqueeze(2) * rays[:, None, 3:6]).reshape(n, 1, -1, 3)
    hom = torch.cat((pts, torch.ones_like(pts[..., :1])), dim=-1)
    cam = net.grid_c_poses_w2c[:, :, :3, :] @ hom.permute(0, 1, 3, 2)
    q = (net.grid_c_Ks @ cam).permute(0, 1, 3, 2)
    xy = q[..., :2] / q[..., 2:3].clamp_min(EPS)
    col = F.grid_sample(frames.view(n * nv, 27, H, W), xy.view(n * nv, 1, -1, 2), mode="bilinear", padding_mode="border", align_corners=False)
    col = col.view(n, nv, 27, -1).permute(0, 3, 1, 2).reshape(z.shape[0], z.shape[1], nv * 27)
    return torch.sum(weights.unsqueeze(-1) * col, -2)


def shape_case(n, rays_per, backward, iters, warmup):
    patch, plain, scene, frames = nets(n)
    g = torch.Generator().manual_seed(1)
    all_rays = native.gen_rays(scene["poses"][:, 0].cuda().contiguous(), scene["projs"][:, 0].cuda().contiguous(), H, W, 3.0, 80.0).view(n, -1, 8)
    pick = torch.randperm(H * W, generator=g)[:rays_per].sort().values.cuda()
    rays = all_rays[:, pick].reshape(-1, 8).contiguous()
    r = bts.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True).cuda().train(backward)
    z = r.sample_coarse(rays)
    g_rgb = {27: torch.randn(rays.shape[0], NV * 27, device="cuda"), 3: torch.randn(rays.shape[0], NV * 3, device="cuda")}

    def render(net, ch):
        def fn():
            with torch.set_grad_enabled(backward):
                comp = r.composite(net, rays, z, coarse=True, sb=n, want_alphas=False, want_rgb_samps=False)
                if backward:
                    torch.autograd.grad((comp[1] * g_rgb[ch]).sum(), [net.encoder.feats[0]] + list(net.mlp_coarse.parameters()))
        return fn

    ft = patch.native_field()
    with torch.no_grad():
        weights = r.composite(patch, rays, z, coarse=True, sb=n)[0].detach()

    def colours():
        rgb, _ = native.patch_color_fwd(ft, rays, z, weights)
        if backward:
            native.patch_color_bwd(ft, rays, z, g_rgb[27])
        return rgb

    def eager():
        w = weights.clone().requires_grad_(backward)
        with torch.set_grad_enabled(backward):
            rgb = eager_colours(frames, patch, rays, z, w)
            if backward:
                torch.autograd.grad((rgb * g_rgb[27]).sum(), w)
        return rgb.detach()

    err = (colours() - eager()).abs().max().item()
    if not err <= 1e-5:
        sys.exit(f"patch_color_probe: the two colour routes differ by {err:.3e} (bar 1e-5)")
    t = dict(patch=[], plain=[], colours=[], eager=[])
    for _ in range(4):
        t["patch"].append(mean_ms(render(patch, 27), iters // 4, warmup // 4 + 1))
        t["plain"].append(mean_ms(render(plain, 3), iters // 4, warmup // 4 + 1))
        t["colours"].append(mean_ms(colours, iters // 4, warmup // 4 + 1))
        t["eager"].append(mean_ms(eager, max(4, iters // 20), 2))
    out = dict(rays=rays.shape[0], backward=backward, rgb_max_diff=err)
    for k, v in t.items():
        out[k] = round(sum(v) / 4, 4)
        out[k + "_blocks"] = [round(x, 4) for x in v]
    out["added_by_27_channels"] = round(out["patch"] - out["plain"], 4)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("patch_color_probe: no GPU; nothing is measured without one")
    res = dict(metric="ms_per_call", size=[H, W], K=K, nv=NV, iters=args.iters, warmup=args.warmup,
               train=shape_case(16, 4096, True, args.iters, args.warmup), frame=shape_case(1, H * W, False, args.iters, args.warmup))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("Patch colours (27 channels per render view), ms per call (tools/patch_color_probe.py; HIP events, mean over "
                    f"{res['iters']} iterations after {res['warmup']} warm-ups, four alternated blocks)\n")
            for case in ("train", "frame"):
                f.write(f"{case}:\n")
                for k, v in res[case].items():
                    f.write(f"  {k:40s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
