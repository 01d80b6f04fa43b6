"""ms per frame of a novel-view video frame (render_poses + the frame lines of gen_vid_nvs.py: image over colour-mapped depth) at
192 x 640, K = 64, a trajectory of 8 poses of one encoded field.  Times, in ONE process,

  fused          FusedNovelViews.frames over the 8 poses (one bts_novel_views call: rays, render with the invalid_wsum epilogue, frame
                 maximum, finish), per frame
  rays           bts_gen_rays for the 8 poses, per frame
  render_epi     the render at the same rays and jitter with the epilogue's invalid_wsum (what the fused call launches), per frame
  render_bare    the same render with rgb and depth only -- the number to report is added_over_bare_render = fused - render_bare
  finish         the frame maximum + the finish kernel on a held render (finish_views), per frame
  host           the reference's route restated on the same GPU, per frame: the render with weights / alphas / invalid, two
                 device-to-host copies of whole images, the mask and the normalisation on the host, matplotlib's colour map, the
                 concatenation and the uint8 conversion
  color_tensor   color_tensor alone at 192 x 640 on the device against the host round trip (copy, matplotlib in numpy, copy back)

with HIP events over --iters iterations after --warmup warm-ups (mean of the timed window; the host routes end in their own copies).
fused, render_bare and host are alternated in four blocks, so that a drifting clock meets all of them; the block means are printed.
Prints ONE JSON line and, with --out, writes the same numbers as text.

    python tools/novel_views_probe.py [--out profiles/r14a/novel_views.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from behindthescenes_amd import native, novel_views as NV, synthetic  # noqa: E402

H, W, C, HD, K, P = 192, 640, 64, 64, 64, 8
D_MIN, D_MAX = 3.0, 80.0


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


def setup():
    scene = synthetic.synthetic_scene(1, 1, H, W, C, seed=9, intrinsics=synthetic.K_KITTIRAW, smooth=True)
    torch.manual_seed(4)
    net = bts.BTSNet(synthetic.field_conf(C, HD, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), C, num_views=1)
    synthetic.init_mlp_(net.mlp_coarse, seed=7)
    net = net.cuda().eval()
    wrapped = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=True)).bind_parallel(net).eval().cuda()
    images, projs, poses = (scene[k].cuda() for k in ("images", "projs", "poses"))
    net.encode(images, projs, poses, ids_encoder=[0], ids_render=[0])
    net.set_scale(0)
    traj = torch.eye(4).repeat(P, 1, 1)
    traj[:, 0, 3] = torch.linspace(0.0, 0.5, P)          # a sideways dolly with a slight yaw
    for i in range(P):
        a = 0.02 * i
        traj[i, 0, 0], traj[i, 0, 2], traj[i, 2, 0], traj[i, 2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return wrapped, net, traj.cuda(), projs[0, 0].contiguous()


def host_frame(wrapped, smp, pose, proj, cmap):
    """render_poses (scripts/inference_setup.py:182-198) and the frame lines of gen_vid_nvs.py:105-120, restated"""
    rays, _ = smp.sample(None, pose.view(1, 1, 4, 4), proj.view(1, 1, 3, 3))
    rd = wrapped(rays, want_weights=True, want_alphas=True)
    rd["fine"] = dict(rd["coarse"])
    c = smp.reconstruct(rd)["coarse"]
    depth = c["depth"].squeeze(1)[0].cpu()
    frame = c["rgb"][0].cpu()
    invalid = (c["invalid"].squeeze(-1) * c["weights"]).sum(-1).squeeze() > .8      # (never applied without black_invalid, as there)
    img = frame[0, :, :, 0].numpy()
    d = ((1 / depth - 1 / D_MAX) / (1 / D_MIN - 1 / D_MAX)).clamp(0, 1)
    col = cmap(d.numpy())[..., :3]
    return (np.concatenate((img, col), axis=0) * 255).astype(np.uint8), invalid


def run(iters, warmup):
    import matplotlib
    out = dict(metric="ms_per_frame", size=[H, W], K=K, poses=P, iters=iters, warmup=warmup)
    wrapped, net, traj, proj = setup()
    smp = bts.ImageRaySampler(D_MIN, D_MAX, H, W, norm_dir=False)
    nv = bts.FusedNovelViews(wrapped, smp, cmap="magma", poses_per_call=P)
    u = torch.rand(P * H * W, K, device="cuda")
    projs = proj.expand(P, 3, 3).contiguous()
    ft, params = net.native_field(), net.mlp_coarse.packed().detach()
    rays = native.gen_rays(traj, projs, H, W, D_MIN, D_MAX, False).view(-1, 8)
    kw = dict(hard_alpha_cap=True, jitter=u, lindisp=True, want_invalid=False)
    held = native.render_fwd(ft, params, rays, None, want_invalid_sums=True, **kw)
    rgb, depth, wsum = held["rgb"].view(P, H, W, 3), held["depth"].view(P, H, W), held["invalid_wsum"].view(P, H, W)
    canvas = torch.zeros((P, 2 * H, W, 3), device="cuda", dtype=torch.uint8)
    cmap = matplotlib.colormaps["magma"]

    def fused():
        nv.frames(traj, proj, D_MIN, D_MAX, canvas=canvas, offsets=((0, 0), (H, 0)), jitter=u)

    def bare():
        native.render_fwd(ft, params, rays, None, **kw)

    def host():
        for p in range(P):
            host_frame(wrapped, smp, traj[p], proj, cmap)

    out["rays"] = round(mean_ms(lambda: native.gen_rays(traj, projs, H, W, D_MIN, D_MAX, False), iters, warmup) / P, 4)
    out["render_epi"] = round(mean_ms(lambda: native.render_fwd(ft, params, rays, None, want_invalid_sums=True, **kw), iters, warmup) / P, 4)
    out["finish"] = round(mean_ms(lambda: NV.finish_views(rgb, depth, wsum, D_MIN, D_MAX, "magma", False, canvas, ((0, 0), (H, 0))), iters,
                                  warmup) / P, 4)
    t = dict(fused=[], render_bare=[], host=[])
    for _ in range(4):
        t["fused"].append(mean_ms(fused, iters // 4, warmup // 4 + 1) / P)
        t["render_bare"].append(mean_ms(bare, iters // 4, warmup // 4 + 1) / P)
        t["host"].append(mean_ms(host, max(2, iters // 40), 1) / P)
    for k, v in t.items():
        out[k] = round(sum(v) / 4, 4)
        out[k + "_blocks"] = [round(x, 4) for x in v]
    out["added_over_bare_render"] = round(out["fused"] - out["render_bare"], 4)
    # the fused frames against the host route's, with the same jitter the host route cannot take: sizes only
    out["frame_shape"] = list(canvas.shape[1:])
    x = depth[0].contiguous()

    def ct_host():
        return torch.tensor(cmap(x.cpu().numpy()), device=x.device)[..., :3]
    out["color_tensor"] = round(mean_ms(lambda: bts.color_tensor(x, "magma", norm=True), iters, warmup), 4)
    out["color_tensor_host"] = round(mean_ms(ct_host, max(20, iters // 4), max(5, warmup // 5)), 4)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("novel_views_probe: no GPU; nothing is measured without one")
    with torch.no_grad():
        res = run(args.iters, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("Novel-view frames (image over colour-mapped depth), ms per frame (tools/novel_views_probe.py; HIP events, mean over "
                    f"{res['iters']} iterations after {res['warmup']} warm-ups)\n")
            for k, v in res.items():
                f.write(f"{k:44s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
