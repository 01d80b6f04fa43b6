"""Golden fixture for MLP-predicted colour (``sample_color: false``) at the kernels' envelope shapes, FROM THE REAL REFERENCE (imported
unmodified through oracle/ref_shim.py).  Run in the build container only:

    python -B tests/golden/gen_golden_mlp_color.py        ->  tests/golden/mlp_color.npz

Two cases: ``a`` = (C, d_hidden, n_blocks) = (64, 64, 0), code_mode z, learn_empty on; ``b`` = (32, 32, 1), code_mode distance,
learn_empty off.  (empty_empty is not recorded: with sample_color=False the reference's
`sigma[invalid_features[..., 0]] = 0` (models_bts.py:323-324) indexes a (n, P, 1) tensor with an (n, 1, P) mask and raises; the kernels'
empty_empty is pinned to the PyTorch composition in tests/test_gpu_mlp_color.py.)  n = 2 maps of 16 x 32, K = 16, 96 rays per batch element.  b_out[0] is shifted so that 30 % of the
samples have o0 < 0: a dead density with a live colour gradient.  Recorded for each case: NeRFRenderer.composite (eval mode), the field
queries with and without only_density, autograd gradients of a seeded scalar -- each once in fp32 (the anchor) and once with the whole
reference in fp64 (the yardstick of fp32 rounding) -- the per-sample dead-density mask and the texels reached ONLY by dead samples."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from oracle import bts_oracle as O
from oracle.ref_shim import load_reference

torch.set_num_threads(4)

CASES = {  # name: (C, Hd, n_blocks, code_mode, learn_empty, empty_empty, seed)
    "a": (64, 64, 0, "z", True, False, 51),
    "b": (32, 32, 1, "distance", False, False, 52),
}


def conf(C, Hd, nb, code_mode, learn_empty, empty_empty):
    return dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=learn_empty, empty_empty=empty_empty, code_mode=code_mode, sample_color=False,
                code=dict(num_freqs=6, freq_factor=1.5, include_input=True), encoder=dict(type="monodepth2"),
                mlp_coarse=dict(type="resnet", n_blocks=nb, d_hidden=Hd), mlp_fine=dict(type="empty"))


def tap_texels(pts, w2c, K, H, W):
    """(n, P, 3) world points -> (n, P, 4) texel indices y * W + x of the four bilinear taps (grid_sample, border, align_corners=False)
    and the frustum flag (n, P)."""
    hom = torch.cat((pts, torch.ones_like(pts[..., :1])), -1)
    cam = (w2c[:, :3, :] @ hom.transpose(1, 2))
    q = K @ cam
    z = q[:, 2]
    x, y = q[:, 0] / z.clamp_min(1e-3), q[:, 1] / z.clamp_min(1e-3)
    inv = (z <= 1e-3) | (x < -1) | (x > 1) | (y < -1) | (y > 1)
    ix = (((x + 1) * W - 1) / 2).clamp(0, W - 1)
    iy = (((y + 1) * H - 1) / 2).clamp(0, H - 1)
    x0, y0 = ix.floor().long(), iy.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    return torch.stack((y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1), -1), inv


def case(ref, name, out):
    C, Hd, nb, code_mode, learn_empty, empty_empty, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    n, v, H, W, K, B = 2, 3, 16, 32, 16, 96
    scene = O.synthetic_scene(n, v, H, W, C, seed=seed, intrinsics=O.K_KITTI360, yaw_deg=9.0, smooth=True)
    feats = torch.randn(n, C, H, W, generator=g).half().float()        # fp16-representable: stored as fp16, bit-exact in fp32
    net = ref.make_net(conf(C, Hd, nb, code_mode, learn_empty, empty_empty), [feats])
    mlp = net.mlp_coarse
    with torch.no_grad():
        # the reference's own initialisation (kaiming) plus non-zero biases and fc_1 (zero-initialised upstream) so every term is exercised
        for k, p in mlp.named_parameters():
            if k.endswith("bias") or "fc_1" in k:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        if learn_empty:
            net.empty_feature.copy_(torch.randn(C, generator=g))
    renderer = ref.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True)
    net.eval(), renderer.eval()
    net.encode(scene["images"], scene["projs"], scene["poses"], ids_encoder=[0], ids_render=[1, 2])
    rays_all = O.image_rays(scene["poses"][:, :1], scene["projs"][:, :1], H, W, 3.0, 80.0)
    rays = rays_all[:, torch.randperm(rays_all.shape[1], generator=g)[:B].sort().values].contiguous()
    z = O.sample_coarse(rays.reshape(-1, 8), K, True, torch.rand(n * B, K, generator=g))
    pts = (rays.reshape(-1, 8)[:, None, :3] + z.unsqueeze(2) * rays.reshape(-1, 8)[:, None, 3:6]).reshape(n, -1, 3).contiguous()
    # b_out[0]: 30 % of the samples with o0 < 0
    o0 = []
    hook = mlp.register_forward_hook(lambda m, i, o: o0.append(o[..., 0].detach().reshape(-1)))
    with torch.no_grad():
        net(pts)
    hook.remove()
    with torch.no_grad():
        mlp.lin_out.bias[0] -= torch.quantile(o0[0], 0.3)
    net64 = ref.make_net(conf(C, Hd, nb, code_mode, learn_empty, empty_empty), [feats.clone()])
    net64.load_state_dict(net.state_dict())
    net64 = net64.double().eval()
    net64.encode(scene["images"].double(), scene["projs"].double(), scene["poses"].double(), ids_encoder=[0], ids_render=[1, 2])
    g_rgb, g_depth = torch.randn(n * B, 3, generator=g), torch.randn(n * B, generator=g) * 0.1
    # (not stored: the frames -- this head reads none; the query points -- rays + z * direction, recomputed)
    arr = dict(projs=scene["projs"], poses=scene["poses"], feats=feats.half(), rays=rays, z=z, gin_rgb=g_rgb, gin_depth=g_depth)
    if learn_empty:
        arr["empty"] = net.empty_feature
    for k, p in mlp.named_parameters():
        arr["p_" + k.replace(".", "_")] = p
    for tag, m, dt in (("", net, torch.float32), ("f64_", net64, torch.float64)):
        o0 = []
        hook = m.mlp_coarse.register_forward_hook(lambda mod, i, o: o0.append(o[..., 0].detach().reshape(-1)))
        w, rgb, depth, alphas, invalid, _, rgbs = renderer.composite(m, rays.reshape(-1, 8).to(dt), z.to(dt), coarse=True, sb=n)
        hook.remove()
        params = list(m.mlp_coarse.parameters()) + [m.encoder.feats[0]] + ([m.empty_feature] if learn_empty else [])
        grads = torch.autograd.grad((rgb * g_rgb.to(dt)).sum() + (depth * g_depth.to(dt)).sum(), params, allow_unused=True)
        with torch.no_grad():
            q_rgb, q_inv, q_sig = m(pts.to(dt))
            d_rgb, d_inv, d_sig = m(pts.to(dt), only_density=True)
        if not tag:
            arr["rgb_samps"] = rgbs       # (its fp64 yardstick: f64_q_rgb, the same points)
        arr.update({tag + "weights": w, tag + "rgb": rgb, tag + "depth": depth, tag + "alphas": alphas, tag + "invalid": invalid,
                    tag + "q_rgb": q_rgb, tag + "q_invalid": q_inv, tag + "q_sigma": q_sig, tag + "qd_sigma": d_sig,
                    tag + "qd_invalid": d_inv})
        names = [k for k, _ in m.mlp_coarse.named_parameters()] + ["feats"] + (["empty"] if learn_empty else [])
        for k, gr in zip(names, grads):
            arr[tag + "g_" + k.replace(".", "_")] = torch.zeros(1) if gr is None else gr
        if not tag:
            dead = (o0[0] < 0).reshape(n, B * K)
    # texels reached only by dead-density samples (their whole gradient is the colour's): the fixture's sharpest test of the liveness slot
    w2c = torch.inverse(scene["poses"][:, 0])
    taps, inv = tap_texels(pts, w2c, scene["projs"][:, 0], H, W)
    reach = ~(inv & learn_empty)          # learn_empty: an out-of-frustum point reads the empty feature, no texel
    live_tex, dead_tex = torch.zeros(n, H * W, dtype=torch.bool), torch.zeros(n, H * W, dtype=torch.bool)
    for b in range(n):
        live_tex[b, taps[b][reach[b] & ~dead[b]].reshape(-1)] = True
        dead_tex[b, taps[b][reach[b] & dead[b]].reshape(-1)] = True
    arr["dead"] = dead
    arr["dead_only_texels"] = (dead_tex & ~live_tex).reshape(n, H, W)
    # (size: the fp64 results are stored rounded to fp32 -- 2^-24 relative, far below every tolerance that uses them -- and the fp64
    # feature-map gradient as its fp16 difference from the fp32 one)
    arr["f64_g_feats"] = (arr["f64_g_feats"] - arr["g_feats"].double()).half()
    for k, a in arr.items():
        a = a.detach()
        out[f"{name}_{k}"] = a.numpy() if a.dtype in (torch.bool, torch.float16) else a.float().numpy()
    out[f"{name}_meta"] = np.array(repr(dict(n=n, v=v, H=H, W=W, C=C, Hd=Hd, n_blocks=nb, K=K, code_mode=code_mode, learn_empty=learn_empty,
                                             empty_empty=empty_empty, ids_render=[1, 2])))
    print(name, "dead share", dead.float().mean().item(), "dead-only texels", int(arr["dead_only_texels"].sum()), "invalid frac",
          invalid.float().mean().item())


if __name__ == "__main__":
    ref = load_reference()
    out = {}
    for name in CASES:
        case(ref, name, out)
    path = os.path.join(HERE, "mlp_color.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KB")
