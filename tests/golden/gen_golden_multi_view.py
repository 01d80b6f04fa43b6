"""Golden fixture for merged encoder views (``combine_ids`` / several ``ids_encoder``) at the kernels' envelope shapes, FROM THE REAL
REFERENCE (imported unmodified through oracle/ref_shim.py).  Run in the build container only:

    python -B tests/golden/gen_golden_multi_view.py        ->  tests/golden/multi_view.npz

Scene: ``O.synthetic_scene(n=2, v=6, 16 x 32, intrinsics=O.K_KITTI360, yaw_deg=9, smooth=True)``.
``a`` = (64, 64, 0), code_mode z, learn_empty and empty_empty on, K = 16, ids_encoder [4, 2, 0], ids_render [5, 3, 1], combine_ids
[(4, 2), (5, 3)]: one merged pair with the far view first, one single that the reference counts twice.  ``b`` = (32, 32, 1), code_mode
distance, learn_empty off, K = 48, ids_encoder [2, 0], ids_render [1, 3], no combine_ids: the plain mean.  90 rays per batch element,
random interior pixels of views 0 and 3.  b_out[0] is shifted so that 30 % of the samples have o0 < 0.  Recorded: NeRFRenderer.composite
(eval mode), the field query at the same points, autograd gradients of a seeded scalar in rgb and depth -- each in fp32 (the anchor) and
with the whole reference in fp64 (the yardstick of fp32 rounding).

Asserted here, on the reference alone: fp32 and fp64 frustum flags agree at every point and view; no point lies within 1e-5 (normalised
units) of a frustum border or of z = EPS in any view; in every merged group each branch of the pick (first member valid / second picked
/ all invalid) holds >= 5 % of the points.  And on behindthescenes_amd.torch_modes: the composition meets the GPU test's bars on this
data, and its mutants -- singles counted once, last member on ties, all instead of any, colour singles counted twice -- do not.  (The
fifth, "divisor V instead of T", is the composition itself on these two cases: T = 1 + 2 = V = 3 in ``a``, T = V = 2 in ``b``; it is
asserted to be exactly that, and tests/test_multi_view_cpu.py pins T on group patterns where the two differ.)

Storage (the file must stay below 1 MiB): maps and frames are fp16-representable (multiples of 1/2 and of 1/128) and stored as fp16; the
jitter is fp16-representable and stored instead of the depths (``O.sample_coarse`` gives them back bit for bit); fp64 results are scaled
fp16 differences from the fp32 ones; the field query's colours are the composite's rgb_samps (the same points) and are not stored twice,
and rgb_samps -- bilinear taps of frames in [0, 1] -- has no fp64 twin: it is held to the absolute bar alone.  The feature-map gradient
(n V x C x 16 x 32 values, most of the file otherwise) is stored as its product with C / 4 Walsh functions of the channel index
(``tests/_multi_view_fixture.py``: +-1 rows that separate every pair of channels), per view, batch element and texel: the test applies the same product."""
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
from tests._multi_view_fixture import walsh_rows

torch.set_num_threads(4)

EPS = 1e-3
DIFF_SCALE = 2.0 ** 20     # fp64 - fp32 differences are stored as fp16 of (difference * DIFF_SCALE)
CASES = {  # name: (C, Hd, n_blocks, code_mode, learn_empty, empty_empty, K, ids_encoder, ids_render, combine_ids, seed)
    "a": (64, 64, 0, "z", True, True, 16, [4, 2, 0], [5, 3, 1], [(4, 2), (5, 3)], 61),
    "b": (32, 32, 1, "distance", False, False, 48, [2, 0], [1, 3], None, 62),
}


def conf(C, Hd, nb, code_mode, learn_empty, empty_empty):
    return dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=learn_empty, empty_empty=empty_empty, code_mode=code_mode, sample_color=True,
                code=dict(num_freqs=6, freq_factor=1.5, include_input=True), encoder=dict(type="monodepth2"),
                mlp_coarse=dict(type="resnet", n_blocks=nb, d_hidden=Hd), mlp_fine=dict(type="empty"))


def view_flags(pts, poses_c2w, Ks, dt):
    """(n, P, 3), (n, V, 4, 4), (n, V, 3, 3) -> frustum flags (n, V, P) and the distance (n, V, P) to the nearest frustum border / z = EPS"""
    pts, w2c, Ks = pts.to(dt), torch.inverse(poses_c2w.to(dt)), Ks.to(dt)
    hom = torch.cat((pts, torch.ones_like(pts[..., :1])), -1).unsqueeze(1)
    pix = (Ks @ (w2c[:, :, :3, :] @ hom.transpose(-1, -2))).transpose(-1, -2)
    z = pix[..., 2]
    x, y = pix[..., 0] / z.clamp_min(EPS), pix[..., 1] / z.clamp_min(EPS)
    flags = (z <= EPS) | (x < -1) | (x > 1) | (y < -1) | (y > 1)
    dist = torch.stack(((x - 1).abs(), (x + 1).abs(), (y - 1).abs(), (y + 1).abs(), (z - EPS).abs()), -1).amin(-1)
    return flags, dist


def groups_of(v, ids_encoder, ids_render, combine_ids):
    import behindthescenes_amd as bts
    return bts.BTSNet._view_groups(v, ids_encoder, ids_render, combine_ids)


def within_bars(got, ref, ref64):
    """the bars of tests/test_gpu_multi_view.py on (weights, rgb, depth, alphas, invalid, rgb_samps): -> the name of the first one missed"""
    if tuple(got["invalid"].shape) != tuple(ref["invalid"].shape) or not torch.equal(got["invalid"].float(), ref["invalid"].float()):
        return "invalid"
    if ((got["depth"] - ref["depth"]).abs() / ref["depth"].abs().clamp_min(1e-6)).max().item() > 1e-4:
        return "depth"
    for k in ("rgb", "weights", "alphas", "rgb_samps"):
        g, r32, r64 = got[k].double(), ref[k].double(), ref64[k].double()
        e = (g - r32).abs()
        if not (bool((e <= 1e-5).all()) or (k != "rgb_samps" and (g - r64).abs().max().item() <= 1.5 * (r32 - r64).abs().max().item() + 1e-5)):
            return k
    return None


def composition(t, meta, mutant=None):
    """behindthescenes_amd.torch_modes on the CPU over the recorded inputs, optionally with one rule of the merge changed"""
    import behindthescenes_amd as bts
    from behindthescenes_amd import torch_modes as tm
    orig = (tm._merge_groups, tm.sample_features, tm.sample_colors)

    def merge_last_on_ties(values, outside, groups, singles_twice):
        vals, flags = [], []
        for g in groups:
            if len(g) == 1:
                vals.append(values[:, g]), flags.append(outside[:, g])
                if not singles_twice:
                    continue
            o, v = outside[:, g], values[:, g]
            order = torch.arange(len(g) - 1, -1, -1, dtype=torch.int32).view(1, -1, 1, 1)
            pick = (o.to(torch.int32) * len(g) + order).argmin(dim=1, keepdim=True)
            flags.append(torch.gather(o, 1, pick)), vals.append(torch.gather(v, 1, pick.expand(-1, -1, -1, v.shape[-1])))
        return torch.cat(vals, dim=1), torch.cat(flags, dim=1)

    def features(net, xyz, single=True, once=False, use_all=False, by_views=False):
        if once:
            tm._merge_groups = lambda v, o, g, singles_twice: orig[0](v, o, g, False)
        try:
            feats, outside = orig[1](net, xyz, single=False)
        finally:
            tm._merge_groups = orig[0]
        V = net.grid_f_features[net._scale].shape[1]
        mean = feats.sum(dim=1) / V if by_views else feats.mean(dim=1)
        return mean, (torch.all(outside, dim=1) if use_all else torch.any(outside, dim=1))

    if mutant == "singles_once":
        tm.sample_features = lambda net, xyz, single=True: features(net, xyz, once=True)
    elif mutant == "last_on_ties":
        tm._merge_groups = merge_last_on_ties
    elif mutant == "all_not_any":
        tm.sample_features = lambda net, xyz, single=True: features(net, xyz, use_all=True)
    elif mutant == "divisor_views":
        tm.sample_features = lambda net, xyz, single=True: features(net, xyz, by_views=True)
    elif mutant == "colour_singles_twice":
        def colours(net, xyz):
            cols, outside = tm._tap(net.grid_c_imgs, tm._to_views(xyz, net.grid_c_poses_w2c, net.grid_c_Ks)[0]), \
                tm._to_views(xyz, net.grid_c_poses_w2c, net.grid_c_Ks)[3]
            if net.grid_c_combine is not None:
                cols, outside = orig[0](cols, outside, net.grid_c_combine, True)
            return cols, outside
        tm.sample_colors = colours
    try:
        c = dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=meta["learn_empty"], empty_empty=meta["empty_empty"], code_mode=meta["code_mode"],
                 code=dict(num_freqs=6, freq_factor=1.5, include_input=True),
                 encoder=dict(type="feature_map", size=(meta["H"], meta["W"]), d_out=meta["C"], num_views=t["feats"].shape[0]),
                 mlp_coarse=dict(type="resnet", n_blocks=meta["n_blocks"], d_hidden=meta["Hd"]), mlp_fine=dict(type="empty"))
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            net = bts.BTSNet(c)
            with torch.no_grad():
                net.encoder.feats[0].copy_(t["feats"].float())
                for k, p in net.mlp_coarse.named_parameters():
                    p.copy_(t["p_" + k.replace(".", "_")])
                if meta["learn_empty"]:
                    net.empty_feature.copy_(t["empty"])
            net = net.eval()
            net.encode(t["images"].float(), t["projs"], t["poses"], ids_encoder=meta["ids_encoder"], ids_render=meta["ids_render"],
                       combine_ids=meta["combine_ids"])
            r = bts.NeRFRenderer(n_coarse=meta["K"], lindisp=True, hard_alpha_cap=True).eval()
            with torch.no_grad():
                w, rgb, depth, alphas, invalid, _, rgbs = r.composite(net, t["rays"].reshape(-1, 8), t["z"], coarse=True, sb=meta["n"])
        return dict(weights=w, rgb=rgb, depth=depth, alphas=alphas, invalid=invalid, rgb_samps=rgbs)
    finally:
        tm._merge_groups, tm.sample_features, tm.sample_colors = orig


def case(ref, name, out):
    C, Hd, nb, code_mode, learn_empty, empty_empty, K, ids_encoder, ids_render, combine_ids, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    n, v, H, W, B = 2, 6, 16, 32, 90
    V = len(ids_encoder)
    scene = O.synthetic_scene(n, v, H, W, C, seed=seed, intrinsics=O.K_KITTI360, yaw_deg=9.0, smooth=True)
    images = (scene["images"] * 128).round() / 128                       # fp16-representable: stored as fp16, bit-exact in fp32
    # a coarse grid of values (multiples of 1/2): fp16-representable and small once compressed; rows in the reference's order b * V + v
    feats = (torch.randn(n * V, C, H, W, generator=g) * 2).round() / 2
    net = ref.make_net(conf(C, Hd, nb, code_mode, learn_empty, empty_empty), [feats])
    mlp = net.mlp_coarse
    with torch.no_grad():
        for k, p in mlp.named_parameters():
            if k.endswith("bias") or "fc_1" in k:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        if learn_empty:
            net.empty_feature.copy_(torch.randn(C, generator=g))
    renderer = ref.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True)
    net.eval(), renderer.eval()
    enc = dict(ids_encoder=ids_encoder, ids_render=ids_render, combine_ids=combine_ids)
    net.encode(images, scene["projs"], scene["poses"], **enc)
    # rays: random interior pixels (no outermost row or column: those lie ON the frustum border of their own view) of views 0 and 3
    rays_all = O.image_rays(scene["poses"][:, [0, 3]], scene["projs"][:, [0, 3]], H, W, 3.0, 80.0).reshape(n, 2, H, W, 8)
    interior = rays_all[:, :, 1:-1, 1:-1].reshape(n, -1, 8)
    rays = interior[:, torch.randperm(interior.shape[1], generator=g)[:B].sort().values].contiguous()
    u = torch.rand(n * B, K, generator=g).half().float().clamp(max=1 - 2.0 ** -11)
    z = O.sample_coarse(rays.reshape(-1, 8), K, True, u)
    pts = (rays.reshape(-1, 8)[:, None, :3] + z.unsqueeze(2) * rays.reshape(-1, 8)[:, None, 3:6]).reshape(n, -1, 3).contiguous()

    # ---- the reference alone: flags in fp32 = fp64, no point at a border, every branch of every merged group populated
    for ids in (ids_encoder, ids_render):
        f32, _ = view_flags(pts, scene["poses"][:, ids], scene["projs"][:, ids], torch.float32)
        f64, dist = view_flags(pts, scene["poses"][:, ids], scene["projs"][:, ids], torch.float64)
        assert torch.equal(f32, f64), f"{name}: fp32 and fp64 frustum flags differ at {int((f32 != f64).sum())} (point, view) pairs"
        print(name, "views", ids, "smallest border distance", dist.min().item())
        assert dist.min().item() >= 1e-5, f"{name}: a point lies within 1e-5 of a frustum border (seed {seed})"
    enc_groups, ren_groups = groups_of(v, ids_encoder, ids_render, combine_ids)
    for ids, groups in ((ids_encoder, enc_groups), (ids_render, ren_groups)):
        flags, _ = view_flags(pts, scene["poses"][:, ids], scene["projs"][:, ids], torch.float64)
        for grp in groups or []:
            if len(grp) < 2:
                continue
            o0, o1 = flags[:, grp[0]], flags[:, grp[1]]
            shares = [(~o0).float().mean().item(), (o0 & ~o1).float().mean().item(), (o0 & o1).float().mean().item()]
            print(name, "group", grp, "first valid / second picked / all invalid:", [round(s, 3) for s in shares])
            assert min(shares) >= 0.05, f"{name}: a branch of group {grp} holds less than 5 % of the points (seed {seed})"

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
    net64.encode(images.double(), scene["projs"].double(), scene["poses"].double(), **enc)
    arr = dict(images=images.half(), projs=scene["projs"], poses=scene["poses"], feats=feats.half(), rays=rays, u=u.half())
    if learn_empty:
        arr["empty"] = net.empty_feature
    for k, p in mlp.named_parameters():
        arr["p_" + k.replace(".", "_")] = p
    res = {}
    for tag, m, dt in (("", net, torch.float32), ("f64_", net64, torch.float64)):
        w, rgb, depth, alphas, invalid, _, rgbs = renderer.composite(m, rays.reshape(-1, 8).to(dt), z.to(dt), coarse=True, sb=n)
        if not tag:
            g_rgb, g_depth = torch.randn(rgb.shape, generator=g), torch.randn(depth.shape, generator=g) * 0.1
            arr["gin_rgb"], arr["gin_depth"] = g_rgb, g_depth
        params = list(m.mlp_coarse.parameters()) + [m.encoder.feats[0]] + ([m.empty_feature] if learn_empty else [])
        grads = torch.autograd.grad((rgb * g_rgb.to(dt)).sum() + (depth * g_depth.to(dt)).sum(), params, allow_unused=True)
        with torch.no_grad():
            q_rgb, q_inv, q_sig = m(pts.to(dt))
        if not tag:   # (not stored twice)
            assert torch.equal(q_rgb.reshape(rgbs.shape), rgbs) and torch.equal(q_inv.reshape(invalid.shape), invalid)
        res[tag] = dict(weights=w, rgb=rgb, depth=depth, alphas=alphas, invalid=invalid, rgb_samps=rgbs, q_sigma=q_sig)
        names = [k for k, _ in m.mlp_coarse.named_parameters()] + ["feats"] + (["empty"] if learn_empty else [])
        for k, gr in zip(names, grads):
            res[tag]["g_" + k.replace(".", "_")] = torch.zeros(1, dtype=dt) if gr is None else gr
        res[tag]["g_feats"] = torch.einsum("rc,mchw->mrhw", walsh_rows(C).to(dt), res[tag]["g_feats"])
    assert torch.equal(res[""]["invalid"], res["f64_"]["invalid"].float())
    for k, a in res[""].items():
        arr[k] = a
        if k not in ("invalid", "rgb_samps"):
            arr["f64_" + k] = ((res["f64_"][k] - a.double()) * DIFF_SCALE).half()
            assert bool(torch.isfinite(arr["f64_" + k]).all()), k
    meta = dict(n=n, v=v, H=H, W=W, C=C, Hd=Hd, n_blocks=nb, K=K, code_mode=code_mode, learn_empty=learn_empty, empty_empty=empty_empty,
                diff_scale=DIFF_SCALE, **enc)

    # ---- the composition and its mutants against the bars
    t = dict({k: a.detach() for k, a in arr.items()}, z=z)
    ref32 = {k: a.detach() for k, a in res[""].items()}
    ref64 = {k: a.detach() for k, a in res["f64_"].items()}
    miss = within_bars(composition(t, meta), ref32, ref64)
    assert miss is None, f"{name}: the composition itself misses the bar on {miss}"
    missed = {}
    for mutant in ("singles_once", "last_on_ties", "all_not_any", "divisor_views", "colour_singles_twice"):
        try:
            missed[mutant] = within_bars(composition(t, meta, mutant), ref32, ref64)
        except RuntimeError as e:      # (a third colour view does not even fit the composition's own output shape)
            missed[mutant] = f"raises {type(e).__name__}"
    print(name, "mutants leave the bars at:", missed)
    assert missed["divisor_views"] is None      # T = V on this data (the module docstring)
    assert missed["all_not_any"] is not None
    if combine_ids is not None:
        assert all(missed[m] is not None for m in ("singles_once", "last_on_ties", "colour_singles_twice")), missed

    for k, a in arr.items():
        a = a.detach()
        out[f"{name}_{k}"] = a.numpy() if a.dtype in (torch.bool, torch.float16) else a.float().numpy()
    out[f"{name}_meta"] = np.array(repr(meta))
    print(name, "share of o0 < 0", (o0[0] < torch.quantile(o0[0], 0.3)).float().mean().item(), "invalid frac", invalid.float().mean().item())


if __name__ == "__main__":
    ref = load_reference()
    out = {}
    for name in CASES:
        case(ref, name, out)
    path = os.path.join(HERE, "multi_view.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KB")
