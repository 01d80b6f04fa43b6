"""ms per call of MLP-predicted colour (sample_color: false) on the HIP kernels (native_mlp_color: true), the PyTorch composition of
torch_modes.py, and the sampled-colour kernels (sample_color: true) for context.  Prints ONE JSON line.

    python tools/mlp_color_bench.py [--reps N]

Shapes: the eval_depth frame (1 x 192 x 640 rays, K = 64, (C, Hd, n_blocks) = (64, 64, 0), forward); exp_kitti_raw.yaml's per-GPU batch
(8 x 2 048 rays, K = 64, (64, 64, 0), forward + backward); exp_re10k.yaml's (24 x 1 024 rays, K = 48, (32, 32, 1), forward + backward).
Timed with HIP events after >= 25 ms of continuous warm-up work (profiles/r06q: the device needs that long to reach steady state)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from behindthescenes_amd import synthetic  # noqa: E402

SHAPES = {   # name: (n, rays per element, K, C, Hd, n_blocks, H, W, backward)
    "eval_frame_fwd": (1, 192 * 640, 64, 64, 64, 0, 192, 640, False),
    "kitti_raw_fwd_bwd": (8, 2048, 64, 64, 64, 0, 192, 640, True),
    "re10k_fwd_bwd": (24, 1024, 48, 32, 32, 1, 256, 384, True),
}


def _net(mode, n, C, Hd, nb, H, W):
    conf = dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=False, code_mode="z", sample_color=(mode == "sampled"),
                native_mlp_color=(mode == "native"), code=dict(num_freqs=6, freq_factor=1.5, include_input=True),
                encoder=dict(type="feature_map", size=(H, W), d_out=C), mlp_coarse=dict(type="resnet", n_blocks=nb, d_hidden=Hd),
                mlp_fine=dict(type="empty"))
    g = torch.Generator().manual_seed(0)
    net = bts.BTSNet(conf)
    with torch.no_grad():
        net.encoder.feats[0].data = torch.randn((n, C, H, W), generator=g) * 0.5
        for p in net.mlp_coarse.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if p.dim() > 1 else 0.05))
    return net.cuda()


def _scene(n, H, W, C):
    s = synthetic.synthetic_scene(n, 3, H, W, C, seed=0, smooth=True)
    return s["images"].cuda(), s["projs"].cuda(), s["poses"].cuda()


def _time(fn, reps):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    # warm-up: at least ~25 ms of CONTINUOUS work -- a probe call sizes a batch that is then enqueued without a synchronisation in between
    w0 = torch.cuda.Event(enable_timing=True)
    w1 = torch.cuda.Event(enable_timing=True)
    w0.record()
    fn()
    w1.record()
    w1.synchronize()
    batch = max(3, int(40.0 / max(w0.elapsed_time(w1), 1e-3)) + 1)
    for _ in range(batch):
        fn()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def run(reps):
    out = {}
    for name, (n, B, K, C, Hd, nb, H, W, bwd) in SHAPES.items():
        imgs, projs, poses = _scene(n, H, W, C)
        g = torch.Generator(device="cuda").manual_seed(1)
        rays = torch.empty((n * B, 8), device="cuda")
        rays[:, :3] = torch.randn((n * B, 3), device="cuda", generator=g) * 0.05
        d = torch.randn((n * B, 3), device="cuda", generator=g) * 0.3
        d[:, 2] = 1.0
        rays[:, 3:6] = d / d.norm(dim=-1, keepdim=True)
        rays[:, 6], rays[:, 7] = 3.0, 80.0
        u = torch.rand((n * B, K), device="cuda", generator=g)
        z = bts.native.sample_coarse(rays, u, True)
        res = {}
        for mode in ("torch", "native", "sampled"):
            net = _net(mode, n, C, Hd, nb, H, W)
            net.train(bwd)
            r = bts.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True).cuda()

            def step():
                net.encode(imgs, projs, poses, ids_encoder=[0], ids_render=[1, 2])
                with torch.set_grad_enabled(bwd):
                    comp = r.composite(net, rays, z, coarse=True, sb=n, want_weights=False, want_alphas=False, want_rgb_samps=bwd,
                                       want_invalid=False)
                    if bwd:
                        (comp[1].square().mean() + 0.01 * comp[2].mean()).backward()
            try:
                res[mode] = round(_time(step, reps), 4)
            except (RuntimeError, bts.native.BtsNativeError) as e:   # (the torch composition can run out of memory at these shapes)
                res[mode] = f"failed: {str(e).splitlines()[0][:120]}"
            del net
            torch.cuda.empty_cache()
        out[name] = res
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    print(json.dumps(dict(metric="ms_per_call", **run(a.reps))))
