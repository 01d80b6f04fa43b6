"""Golden fixture for patch colours (``image_processor: {type: patch}``, 27-channel colour targets) FROM THE REAL REFERENCE (imported
unmodified through oracle/ref_shim.py; ``PatchProcessor`` from ``models.bts.model.image_processor``).  Run in the build container only:

    python -B tests/golden/gen_golden_patch_color.py        ->  tests/golden/patch_color.npz

Scene: ``O.synthetic_scene(n=2, v=4, 16 x 32, intrinsics=O.K_KITTI360, yaw_deg=9, smooth=True)``, frames fp16-representable.
``a`` = (64, 64, 0), code_mode z, learn_empty, K = 16, ids_render [1, 2, 3].  ``b`` = (32, 32, 1), code_mode distance, K = 48, ids_render
[2], white_bkgd, empty_empty and no hard_alpha_cap (a ray that ends outside the encoder view has weights that sum to less than 1: the background shows).  Encoder view 0; 90 rays per batch element, random interior pixels of all four views.  Recorded, in fp32 (the anchor)
and with the whole reference in fp64 (the yardstick of fp32 rounding): PatchProcessor(3)'s output; NeRFRenderer.composite's rgb, depth,
weights, invalid on ``encode(images_alt=PatchProcessor(3)(images))``; rgb_samps for the first RS rays of each batch element; autograd
gradients of a seeded scalar in rgb and depth w.r.t. the MLP, the maps and the empty feature; the reference's ReconstructionLoss (l2
weight_guided, l1 strict, l2 none) on the render dict of the first 64 rays of each batch element as one 8 x 8 patch with a random
27-channel target, and its gradient in rgb; and one training step on those rays -- their render, l2 under weight_guided, the loss and its
gradient in the MLP and the empty feature.

Asserted here, on the reference alone: in every render view >= 10 % of the samples lie inside the frame within 1.5 texels of its border
and >= 10 % outside the frustum (the ray draw is repeated with the next seed until both hold); no sample within 1e-5 (normalised) of a
frustum border or of a texel boundary, fp32 and fp64 flags equal; the centre triple (channels 12..14 of every view) equals the 3-channel
render within 1e-6.  And on tests/_patch_color_oracle.py: it meets the GPU test's bars on this data, and its mutants -- single clamp,
shifts in (x, y) order, zero padding, no background term -- do not.

Storage (< 1 MiB): maps, frames and the processor's output are fp16-representable and stored as fp16; the jitter is stored instead of the
depths; fp64 results are scaled fp16 differences from the fp32 ones; the maps' gradient is stored as its product with C / 4 Walsh functions
of the channel index (tests/_multi_view_fixture.py), as in gen_golden_multi_view.py."""
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
from tests import _patch_color_oracle as PC
from tests._multi_view_fixture import walsh_rows

torch.set_num_threads(4)

EPS = 1e-3
DIFF_SCALE = 2.0 ** 20
RS = 8                    # rays per batch element whose rgb_samps are recorded
LOSSES = (("l2", "weight_guided"), ("l1", "strict"), ("l2", "none"))
CASES = {  # name: (C, Hd, n_blocks, code_mode, learn_empty, K, ids_render, white_bkgd, seed)
    "a": (64, 64, 0, "z", True, 16, [1, 2, 3], False, 71),
    "b": (32, 32, 1, "distance", False, 48, [2], True, 72),
}


def conf(C, Hd, nb, code_mode, learn_empty, empty_empty):
    return dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=learn_empty, empty_empty=empty_empty, code_mode=code_mode, sample_color=True,
                code=dict(num_freqs=6, freq_factor=1.5, include_input=True), encoder=dict(type="monodepth2"),
                mlp_coarse=dict(type="resnet", n_blocks=nb, d_hidden=Hd), mlp_fine=dict(type="empty"))


def view_stats(pts, poses_c2w, Ks, H, W, dt):
    """-> flags (n, V, P), distance to the nearest frustum border / z = EPS, distance (normalised) to the nearest texel boundary where the
    tap is not clamped away, near-border flags (inside the frame, within 1.5 texels of its border)"""
    pts, w2c, Ks = pts.to(dt), torch.inverse(poses_c2w.to(dt)), Ks.to(dt)
    hom = torch.cat((pts, torch.ones_like(pts[..., :1])), -1).unsqueeze(1)
    pix = (Ks @ (w2c[:, :, :3, :] @ hom.transpose(-1, -2))).transpose(-1, -2)
    z = pix[..., 2]
    x, y = pix[..., 0] / z.clamp_min(EPS), pix[..., 1] / z.clamp_min(EPS)
    flags = (z <= EPS) | (x < -1) | (x > 1) | (y < -1) | (y > 1)
    dist = torch.stack(((x - 1).abs(), (x + 1).abs(), (y - 1).abs(), (y + 1).abs(), (z - EPS).abs()), -1).amin(-1)
    ix, iy = ((x + 1) * W - 1) / 2, ((y + 1) * H - 1) / 2
    tex = torch.ones_like(ix)
    for i, size in ((ix, W), (iy, H)):
        live = (i > -1) & (i < size)                        # (elsewhere the clamp decides, far from any boundary)
        d = (i - i.round()).abs() * 2 / size
        tex = torch.minimum(tex, torch.where(live, d, torch.ones_like(d)))
    near = ~flags & ((ix < 1.5) | (ix > W - 2.5) | (iy < 1.5) | (iy > H - 2.5))
    return flags, dist, tex, near


def within_bars(got, ref, ref64):
    """the bars of tests/test_gpu_patch_color.py on rgb and rgb_samps -> the name of the first one missed"""
    for k in ("rgb", "rgb_samps"):
        g, r32, r64 = got[k].double(), ref[k].double(), ref64[k].double()
        if not (bool(((g - r32).abs() <= 1e-5).all()) or (g - r64).abs().max().item() <= 1.5 * (r32 - r64).abs().max().item() + 1e-5):
            return k
    return None


def case(ref, name, out):
    from models.bts.model.image_processor import PatchProcessor
    C, Hd, nb, code_mode, learn_empty, K, ids_render, white, seed = CASES[name]
    n, v, H, W, B = 2, 4, 16, 32, 90
    nv = len(ids_render)
    g = torch.Generator().manual_seed(seed)
    scene = O.synthetic_scene(n, v, H, W, C, seed=seed, intrinsics=O.K_KITTI360, yaw_deg=9.0, smooth=True)
    images = (scene["images"] * 128).round() / 128
    feats = (torch.randn(n, C, H, W, generator=g) * 2).round() / 2
    net = ref.make_net(conf(C, Hd, nb, code_mode, learn_empty, white), [feats])
    mlp = net.mlp_coarse
    with torch.no_grad():
        for k, p in mlp.named_parameters():
            if k.endswith("bias") or "fc_1" in k:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        if learn_empty:
            net.empty_feature.copy_(torch.randn(C, generator=g))
    renderer = ref.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=not white, white_bkgd=white)   # (b: with empty_empty a ray may end short of 1)
    net.eval(), renderer.eval()
    processor = PatchProcessor(3)
    patches = processor(images)
    assert processor.channels == 27 and patches.shape == (n, v, 27, H, W)
    assert torch.equal(patches.half().float(), patches) and torch.equal(processor(images.double()).float(), patches)
    enc = dict(ids_encoder=[0], ids_render=ids_render)

    # ---- rays: interior pixels of all views, each with its own jitter row.  A candidate is dropped when one of its samples lies within 1e-5 of
    # a frustum border or a texel boundary in any view it is seen from, or is flagged differently in fp32 and fp64; of the rest, 20 per
    # render view and batch element are drawn from the 60 with the most samples outside that view, the others at random
    rays_all = O.image_rays(scene["poses"], scene["projs"], H, W, 3.0, 80.0).reshape(n, v, H, W, 8)
    cand = rays_all[:, :, 1:-1, 1:-1].reshape(n, -1, 8)
    M = cand.shape[1]
    views = [0] + ids_render
    for attempt in range(20):
        ga = torch.Generator().manual_seed(seed * 1000 + attempt)
        cu = torch.rand(n * M, K, generator=ga).half().float().clamp(max=1 - 2.0 ** -11)
        cz = O.sample_coarse(cand.reshape(-1, 8), K, True, cu)
        cpts = (cand.reshape(-1, 8)[:, None, :3] + cz.unsqueeze(2) * cand.reshape(-1, 8)[:, None, 3:6]).reshape(n, -1, 3)
        c32, _, _, _ = view_stats(cpts, scene["poses"][:, views], scene["projs"][:, views], H, W, torch.float32)
        c64, cdist, ctex, _ = view_stats(cpts, scene["poses"][:, views], scene["projs"][:, views], H, W, torch.float64)
        ctex[:, 0] = 1.0                                      # (the encoder view's taps are the feature map's: no flag or floor hangs on them here)
        per_ray = lambda t: t.reshape(n, len(views), M, K)
        good = (per_ray(c32 == c64).all(-1).all(1) & (per_ray(cdist).amin(-1).amin(1) >= 1e-5) & (per_ray(ctex).amin(-1).amin(1) >= 1e-5))
        out_frac = per_ray(c64.float())[:, 1:].mean(-1)       # (n, nv, M)
        chosen = []
        for b in range(n):
            ok_ids = torch.nonzero(good[b]).flatten()
            take = set()
            per_view = 20
            for j in range(nv):
                top = ok_ids[torch.argsort(out_frac[b, j, ok_ids], descending=True)[:60]]
                top = top[torch.randperm(len(top), generator=ga)]
                for i in top.tolist():
                    if len(take) >= (j + 1) * per_view:
                        break
                    take.add(i)
            rest = ok_ids[torch.randperm(len(ok_ids), generator=ga)].tolist()
            for i in rest:
                if len(take) >= B:
                    break
                take.add(i)
            chosen.append(torch.tensor(sorted(take)))
        rays = torch.stack([cand[b, chosen[b]] for b in range(n)]).contiguous()
        u = torch.cat([cu.reshape(n, M, K)[b, chosen[b]] for b in range(n)]).contiguous()
        z = O.sample_coarse(rays.reshape(-1, 8), K, True, u)
        pts = (rays.reshape(-1, 8)[:, None, :3] + z.unsqueeze(2) * rays.reshape(-1, 8)[:, None, 3:6]).reshape(n, -1, 3).contiguous()
        f32, _, _, _ = view_stats(pts, scene["poses"][:, ids_render], scene["projs"][:, ids_render], H, W, torch.float32)
        f64, dist, tex, near = view_stats(pts, scene["poses"][:, ids_render], scene["projs"][:, ids_render], H, W, torch.float64)
        e32, _, _, _ = view_stats(pts, scene["poses"][:, [0]], scene["projs"][:, [0]], H, W, torch.float32)
        e64, edist, _, _ = view_stats(pts, scene["poses"][:, [0]], scene["projs"][:, [0]], H, W, torch.float64)
        shares = [(near[:, j].float().mean().item(), f64[:, j].float().mean().item()) for j in range(nv)]
        ok = (torch.equal(f32, f64) and torch.equal(e32, e64) and min(dist.min().item(), edist.min().item()) >= 1e-5 and tex.min().item() >= 1e-5
              and all(a >= 0.10 and b >= 0.10 for a, b in shares))
        if ok:
            break
    assert ok, f"{name}: no ray draw met the conditions"
    print(name, "ray draw", attempt, "per view (near border, outside):", [(round(a, 3), round(b, 3)) for a, b in shares],
          "smallest border / texel distance", dist.min().item(), tex.min().item())

    net64 = ref.make_net(conf(C, Hd, nb, code_mode, learn_empty, white), [feats.clone()])
    net64.load_state_dict(net.state_dict())
    net64 = net64.double().eval()
    arr = dict(images=images.half(), projs=scene["projs"], poses=scene["poses"], feats=feats.half(), rays=rays, u=u.half(), patches=patches.half())
    if learn_empty:
        arr["empty"] = net.empty_feature
    for k, p in mlp.named_parameters():
        arr["p_" + k.replace(".", "_")] = p
    res = {}
    pick = torch.cat([torch.arange(RS) + b * B for b in range(n)])
    for tag, m, dt in (("", net, torch.float32), ("f64_", net64, torch.float64)):
        m.encode(images.to(dt), scene["projs"].to(dt), scene["poses"].to(dt), images_alt=processor(images.to(dt)), **enc)
        w, rgb, depth, alphas, invalid, _, rgbs = renderer.composite(m, rays.reshape(-1, 8).to(dt), z.to(dt), coarse=True, sb=n)
        assert rgb.shape == (n * B, nv * 27) and rgbs.shape == (n * B, K, nv * 27)
        if not tag:
            g_rgb, g_depth = torch.randn(rgb.shape, generator=g), torch.randn(depth.shape, generator=g) * 0.1
            arr["gin_rgb"], arr["gin_depth"] = g_rgb, g_depth
        params = list(m.mlp_coarse.parameters()) + [m.encoder.feats[0]] + ([m.empty_feature] if learn_empty else [])
        grads = torch.autograd.grad((rgb * g_rgb.to(dt)).sum() + (depth * g_depth.to(dt)).sum(), params, allow_unused=True)
        res[tag] = dict(weights=w.detach(), rgb=rgb.detach(), depth=depth.detach(), invalid=invalid.detach(), rgb_samps=rgbs.detach()[pick])
        full_samps = rgbs.detach()
        names = [k for k, _ in m.mlp_coarse.named_parameters()] + ["feats"] + (["empty"] if learn_empty else [])
        for k, gr in zip(names, grads):
            res[tag]["g_" + k.replace(".", "_")] = torch.zeros(1, dtype=dt) if gr is None else gr
        res[tag]["g_feats"] = torch.einsum("rc,mchw->mrhw", walsh_rows(C).to(dt), res[tag]["g_feats"])
        # the centre triple is the 3-channel render
        m.encode(images.to(dt), scene["projs"].to(dt), scene["poses"].to(dt), **enc)
        with torch.no_grad():
            _, rgb3, depth3, _, _, _, _ = renderer.composite(m, rays.reshape(-1, 8).to(dt), z.to(dt), coarse=True, sb=n)
        centre = rgb.detach().reshape(-1, nv, 27)[..., 12:15].reshape(-1, nv * 3)
        err = (centre - rgb3).abs().max().item()
        print(name, tag or "f32_", "centre triple vs the 3-channel render:", err)
        assert err <= 1e-6 and torch.equal(depth3, depth.detach())
        # ---- the reference's loss on the first 64 rays of each batch element as one 8 x 8 patch
        sel = torch.cat([torch.arange(64) + b * B for b in range(n)])
        if not tag:
            arr["loss_gt"] = torch.rand(n, 1, 8, 8, 27, generator=g)
        for crit, policy in LOSSES:
            x = rgb.detach()[sel].reshape(n, 1, 8, 8, nv, 27).clone().requires_grad_(True)
            level = dict(rgb=x, depth=depth.detach()[sel].reshape(n, 1, 8, 8), weights=w.detach()[sel].reshape(n, 1, 8, 8, K),
                         invalid=invalid.detach()[sel].reshape(n, 1, 8, 8, K, nv))
            data = dict(coarse=[level], fine=[dict(level)], rgb_gt=arr["loss_gt"].to(dt))
            loss, ld = ref.ReconstructionLoss(dict(criterion=crit, invalid_policy=policy))(data)
            gx, = torch.autograd.grad(loss, x)
            res[tag][f"loss_{crit}_{policy}"] = torch.stack([loss.detach(), torch.tensor(ld["loss_invalid_ratio"], dtype=dt)])
            res[tag][f"lossg_{crit}_{policy}"] = gx.reshape(n * 64, nv * 27)
            if not tag:
                print(name, crit, policy, "loss", loss.item(), "invalid ratio", ld["loss_invalid_ratio"])
        # ---- one training step on those rays: the render of the patch, l2 under weight_guided, the gradient in the MLP and the empty feature
        m.encode(images.to(dt), scene["projs"].to(dt), scene["poses"].to(dt), images_alt=processor(images.to(dt)), **enc)
        w, rgb, depth, _, invalid, _, _ = renderer.composite(m, rays.reshape(-1, 8)[sel].to(dt), z[sel].to(dt), coarse=True, sb=n)
        level = dict(rgb=rgb.reshape(n, 1, 8, 8, nv, 27), depth=depth.reshape(n, 1, 8, 8), weights=w.reshape(n, 1, 8, 8, K),
                     invalid=invalid.reshape(n, 1, 8, 8, K, nv))
        loss, _ = ref.ReconstructionLoss(dict(criterion="l2", invalid_policy="weight_guided"))(
            dict(coarse=[level], fine=[dict(level)], rgb_gt=arr["loss_gt"].to(dt)))
        step_params = list(m.mlp_coarse.parameters()) + ([m.empty_feature] if learn_empty else [])
        step_names = [k for k, _ in m.mlp_coarse.named_parameters()] + (["empty"] if learn_empty else [])
        res[tag]["step_loss"] = loss.detach().reshape(1)
        for k, gr in zip(step_names, torch.autograd.grad(loss, step_params, allow_unused=True)):
            res[tag]["step_g_" + k.replace(".", "_")] = torch.zeros(1, dtype=dt) if gr is None else gr
    assert torch.equal(res[""]["invalid"], res["f64_"]["invalid"].float())
    for k, a in res[""].items():
        arr[k] = a
        if k != "invalid":
            arr["f64_" + k] = ((res["f64_"][k] - a.double()) * DIFF_SCALE).half()
            assert bool(torch.isfinite(arr["f64_" + k]).all()), k
    meta = dict(n=n, v=v, H=H, W=W, C=C, Hd=Hd, n_blocks=nb, K=K, code_mode=code_mode, learn_empty=learn_empty, white_bkgd=white, hard_alpha_cap=not white, empty_empty=white, B=B, RS=RS,
                diff_scale=DIFF_SCALE, **enc)

    # ---- the oracle and its mutants against the bars
    w2c = torch.inverse(scene["poses"])[:, ids_render]
    Ks = scene["projs"][:, ids_render]
    imgs = (images * .5 + .5)[:, ids_render]
    ref32 = dict(rgb=res[""]["rgb"], rgb_samps=res[""]["rgb_samps"])
    ref64 = dict(rgb=res["f64_"]["rgb"], rgb_samps=res["f64_"]["rgb_samps"])

    def oracle(mutant=None):
        samps = PC.sample_colours(imgs, w2c, Ks, rays.reshape(-1, 8), z, mutant)
        return dict(rgb=PC.composite(res[""]["weights"], samps, white, mutant), rgb_samps=samps[pick])

    miss = within_bars(oracle(), ref32, ref64)
    assert miss is None, f"{name}: the oracle itself misses the bar on {miss}"
    samps64 = PC.sample_colours(imgs.double(), torch.inverse(scene["poses"].double())[:, ids_render], Ks.double(), rays.reshape(-1, 8).double(), z.double())
    print(name, "oracle in fp64 vs the reference in fp64: rgb_samps", (samps64[pick] - ref64["rgb_samps"]).abs().max().item())
    missed = {m: within_bars(oracle(m), ref32, ref64) for m in PC.MUTANTS}
    print(name, "mutants leave the bars at:", missed)
    assert all(missed[m] is not None for m in PC.MUTANTS if m != "no_background") and (missed["no_background"] is not None) == white, missed
    gw = PC.g_weights(arr["gin_rgb"], full_samps.float(), white)
    wr = res[""]["weights"].clone().requires_grad_(True)
    gw_ref, = torch.autograd.grad((PC.composite(wr, full_samps.float(), white) * arr["gin_rgb"]).sum(), wr)
    assert (gw - gw_ref).abs().max().item() <= 1e-5
    for crit, policy in LOSSES:
        sel = torch.cat([torch.arange(64) + b * B for b in range(n)])
        lo, go, bad = PC.pixel_loss(res[""]["rgb"][sel].reshape(-1, nv, 27), arr["loss_gt"].reshape(-1, 27), crit, policy,
                                    res[""]["invalid"][sel], res[""]["weights"][sel])
        # (the reference's fine dict aliases the coarse one: its loss and gradient are twice the term's)
        assert abs(2 * lo.item() - res[""][f"loss_{crit}_{policy}"][0].item()) <= 1e-5, (crit, policy)
        assert (2 * go.reshape(n * 64, -1) - res[""][f"lossg_{crit}_{policy}"]).abs().max().item() <= 1e-4 * res[""][f"lossg_{crit}_{policy}"].abs().max().item()
        assert abs(bad / (n * 64) - res[""][f"loss_{crit}_{policy}"][1].item()) <= 1e-6 or policy == "none"

    for k, a in arr.items():
        a = a.detach()
        out[f"{name}_{k}"] = a.numpy() if a.dtype in (torch.bool, torch.float16) else a.float().numpy()
    out[f"{name}_meta"] = np.array(repr(meta))


if __name__ == "__main__":
    ref = load_reference()
    out = {}
    for name in CASES:
        case(ref, name, out)
    path = os.path.join(HERE, "patch_color.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KB")
