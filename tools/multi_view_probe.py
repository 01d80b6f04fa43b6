"""ms per call of merged encoder views (combine_ids, V = 3 with one merged pair) on the HIP kernels (``native_multi_view: true``) against
the PyTorch composition of torch_modes.py -- the same tree without the key.  Prints ONE JSON line.

    python tools/multi_view_probe.py [--iters 200] [--shapes train,frame]

Shapes, (C, Hd, n_blocks) = (64, 64, 0), maps and frames of 192 x 640:
    train   forward + backward at 8 x 2 048 rays, K = 64
    frame   forward only on one 192 x 640 frame, K = 64
Timed with HIP events: ``iters`` calls per side in four blocks, the two sides alternating block by block (native, composition, native, ...)
after one untimed block of each; per side the median block and the range of the blocks, in ms per call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from behindthescenes_amd import synthetic  # noqa: E402

H, W, C, HD, K = 192, 640, 64, 64, 64
ENC = dict(ids_encoder=[0, 2, 4], ids_render=[1, 3], combine_ids=[(0, 2)])
SHAPES = {"train": (8, 2048, True), "frame": (1, H * W, False)}   # name: (n, rays per element, backward)


def _nets(n):
    V = len(ENC["ids_encoder"])
    conf = dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=True, code_mode="z", code=dict(num_freqs=6, freq_factor=1.5, include_input=True),
                encoder=dict(type="feature_map", size=(H, W), d_out=C, num_views=n * V), mlp_coarse=dict(type="resnet", n_blocks=0, d_hidden=HD),
                mlp_fine=dict(type="empty"))
    g = torch.Generator().manual_seed(0)
    comp = bts.BTSNet(conf)
    with torch.no_grad():
        comp.encoder.feats[0].copy_(torch.randn((n * V, C, H, W), generator=g) * 0.5)
        for p in comp.mlp_coarse.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if p.dim() > 1 else 0.05))
    nat = bts.BTSNet(dict(conf, native_multi_view=True))
    nat.load_state_dict(comp.state_dict())
    return comp.cuda(), nat.cuda()


def _call(net, renderer, scene, rays, u, n, backward):
    images, projs, poses = scene
    z = bts.native.sample_coarse(rays, u, True)

    def fn():
        if not backward:
            with torch.no_grad():
                net.encode(images, projs, poses, **ENC)
                renderer.composite(net, rays, z, sb=n, want_weights=False, want_alphas=False, want_rgb_samps=False)
            return
        net.zero_grad(set_to_none=True)
        net.encode(images, projs, poses, **ENC)
        out = renderer.composite(net, rays, z, sb=n, want_weights=False, want_alphas=False, want_rgb_samps=False)
        (out[1].square().mean() + 0.01 * out[2].mean()).backward()
    return fn


def _block(fn, count):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(count):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--shapes", default="train,frame")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multi_view_probe needs a GPU: nothing is measured without one")
    import warnings
    warnings.simplefilter("ignore")
    out = {}
    for name in args.shapes.split(","):
        n, per, backward = SHAPES[name]
        s = synthetic.synthetic_scene(n, 5, H, W, C, seed=0, smooth=True)
        scene = (s["images"].cuda(), s["projs"].cuda(), s["poses"].cuda())
        all_rays = bts.ImageRaySampler(3.0, 80.0, H, W).sample(None, scene[2][:, :1], scene[1][:, :1])[0].reshape(n, -1, 8)
        pick = torch.randperm(all_rays.shape[1], generator=torch.Generator().manual_seed(1))[:per].sort().values.cuda()
        rays = all_rays[:, pick].reshape(-1, 8).contiguous()
        u = torch.rand((rays.shape[0], K), generator=torch.Generator().manual_seed(2)).cuda()
        comp, nat = _nets(n)
        renderer = bts.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True).cuda()
        for net in (comp, nat):
            net.train(backward), renderer.train(backward)
        fns = {"native": _call(nat, renderer, scene, rays, u, n, backward), "composition": _call(comp, renderer, scene, rays, u, n, backward)}
        per_block = max(1, args.iters // 4)
        for fn in fns.values():            # one untimed block each: code objects, allocator, workspaces
            _block(fn, max(2, per_block // 5))
        blocks = {k: [] for k in fns}
        for _ in range(4):
            for k, fn in fns.items():
                blocks[k].append(_block(fn, per_block))
        rec = {}
        for k, b in blocks.items():
            rec[k] = dict(ms=round(sorted(b)[len(b) // 2], 4), blocks=[round(x, 4) for x in b])
        rec["speedup"] = round(rec["composition"]["ms"] / rec["native"]["ms"], 3)
        out[name] = rec
        del comp, nat
        torch.cuda.empty_cache()
    print(json.dumps(dict(metric="multi_view_ms_per_call", iters=args.iters, V=3, K=K, shape=[C, HD, 0], includes="encode (projection passes) + composite"
                          " [+ backward]", **out)))


if __name__ == "__main__":
    main()
