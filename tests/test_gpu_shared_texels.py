"""The render kernel's second loop (rays whose samples all hit the same four texels of G fetch them ONCE) against the build
without it (variants/libbts_nosharedtexels.so, -DBTS_NO_SHARED_TEXELS): every output bit for bit.

Every sample keeps its own weights, encoding and FMAs in the shared loop; only the source of the rows differs, so the yardstick is
torch.equal, not a tolerance.  Each case first works out ON THE CPU (the oracle's projection + make_taps' index formula) which rays
are of the shared class, and asserts that the classes the case is about are really there: no device counter sits on the hot path.
One child process per library renders all the cases (the library is chosen at load time through BTS_RENDER_LIB)."""
import functools
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, C, HD = 96, 320, 64, 64
RERUNS = 20
# sideways shift of the encoder-view origins in `near_miss`.  A shift of s metres moves a sample at depth z by fx (W / 2) s / z texels:
# 186 s / z here, i.e. 0.31 texels at the near plane (3 m) for s = 5e-3 and nothing at the far end.  The sub-texel phase of the pixel
# columns, j / (W - 1) + 0.5 mod 1, is uniform over a row, so about 0.31 of the rays have near samples across a texel boundary and
# the rest stay shared.  (1e-3 m moves the near samples by 0.06 texels: 6 % of the rays, too few to alternate the loops ray by ray.)
NEAR_MISS_SHIFT = 5e-3

# name: (n, v, K, ids_render, conf, origin shift of the view-0 rays, rays dropped at the end, z from the jitter inside the kernel).
# View 0 is the encoder's: its rays are the shared class, the partner view's (and the shifted ones whose near samples cross a texel
# boundary) the other; every case holds both.
#
# k48 / k33: the library renders 32 < K <= 48 in its 48-lane mode (four rays in three wave iterations, which has no second loop)
# whenever the ray count per batch element is a multiple of 4 (render_geometry, csrc/bts_fwd.hip).  These two cases drop the last ray:
# 61 439 rays are no multiple of 4, so they run one ray per wave with 16 and 31 idle lanes, whose taps are those of sample K - 1 in
# the shared-texel compare, through both loops.
CASES = {
    "eval_like": (1, 2, 64, [0], dict(learn_empty=True), 0.0, 0, False),   # the flagship's structure, all rays (frustum-border pixels included)
    "two_samples": (2, 2, 64, [0], {}, 0.0, 0, False),                     # two batch elements, view0 view1 view0 view1: three switches of loop per wave
    "k48": (1, 2, 48, [0], {}, 0.0, 1, False),                             # one ray per wave with idle lanes (see above)
    "k33": (1, 2, 33, [0], {}, 0.0, 1, False),
    "nv2": (1, 2, 64, [0, 1], {}, 0.0, 0, False),                          # colour taps by the enc_view route and by the other
    "near_miss": (1, 1, 64, [0], {}, NEAR_MISS_SHIFT, 0, False),           # the two loops alternate ray by ray
    "eval_jitter": (1, 2, 64, [0], dict(learn_empty=True), 0.0, 0, True),  # the flagship's route: sample_coarse inside the kernel (z_pre / nrec across a hand-over)
}
NAMES = ("weights", "rgb", "depth", "alphas", "invalid")


def _inputs(name):
    """Scene, rays (n * v * H * W - dropped, 8), z (rays, K) and the jitter u (rays, K) that z was sampled from, of a case, on the
    CPU, from seeds alone: both child processes and the test itself build the same tensors."""
    from behindthescenes_amd import synthetic as S
    from oracle import bts_oracle as O
    n, v, K, ids, conf, shift, drop, in_kernel = CASES[name]
    seed = 300 + list(CASES).index(name)
    g = torch.Generator().manual_seed(seed)
    scene = S.synthetic_scene(n, v, H, W, C, seed=seed, intrinsics=S.K_KITTIRAW, smooth=True)
    rays = O.image_rays(scene["poses"], scene["projs"], H, W, 3.0, 80.0).clone()    # (n, v * H * W, 8), view after view
    if shift:
        rays[:, :H * W, 0] += shift
    rays = rays.reshape(-1, 8)
    rays = rays[:rays.shape[0] - drop].contiguous()
    u = torch.rand(rays.shape[0], K, generator=g)
    return scene, rays, O.sample_coarse(rays, K, True, u), u


def _tap_indices(xy):
    """make_taps' texel indices (bts_common.h) of image coordinates xy (..., 2) in [-1, 1]: (..., 3) = o00, o01, o10."""
    ix = ((xy[..., 0] + 1.0) * W - 1.0) / 2.0
    iy = ((xy[..., 1] + 1.0) * H - 1.0) / 2.0
    ix, iy = ix.clamp(0.0, W - 1.0), iy.clamp(0.0, H - 1.0)
    x0, y0 = ix.floor().long(), iy.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    return torch.stack((y0 * W + x0, y0 * W + x1, y1 * W + x0), -1)


@functools.lru_cache(maxsize=None)
def shared_class(name):
    """(rays,) bool: all K samples of the ray project onto the same taps of the encoder view's map."""
    from oracle import bts_oracle as O
    n = CASES[name][0]
    scene, rays, z, _ = _inputs(name)
    r = rays.view(n, -1, 8)
    pts = r[:, :, None, 0:3] + z.view(n, r.shape[1], -1, 1) * r[:, :, None, 3:6]
    w2c = torch.linalg.inv(scene["poses"][:, :1])
    xy = O.project(pts.reshape(n, -1, 3), w2c, scene["projs"][:, :1])[0][:, 0]
    taps = _tap_indices(xy).view(n * r.shape[1], z.shape[1], 3)
    return (taps == taps[:, :1]).all(-1).all(-1)


CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
import behindthescenes_amd as bts
from behindthescenes_amd import synthetic as S
from tests.test_gpu_shared_texels import CASES, RERUNS, _inputs
out = dict()
with torch.no_grad():
    for name, (n, v, K, ids, conf, shift, drop, in_kernel) in CASES.items():
        scene, rays, z, u = _inputs(name)
        torch.manual_seed(11)   # BTSNet draws its empty_feature from the global generator: the same in both processes
        net = S.build_net(scene, d_hidden={hd}, n_blocks=0, ids_render=ids, device="cuda", mlp_seed=11, **conf)
        renderer = bts.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True).cuda().eval()
        rays, z, u = rays.cuda(), z.cuda(), u.cuda()
        if in_kernel:   # z_samp None: the kernel samples the depths itself from u
            render = lambda: renderer._composite(net, rays, None, True, n, True, True, False, True, False, jitter=u)[:5]
        else:
            render = lambda: renderer.composite(net, rays, z, sb=n, want_rgb_samps=False)[:5]
        first = render()
        out[name] = [t.cpu() for t in first]
        if name == "eval_like":
            same = True
            for _ in range(RERUNS - 1):
                again = render()
                same = same and all(torch.equal(a, b) for a, b in zip(first, again))
            out["rerun"] = same
torch.save(out, sys.argv[1])
"""


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    """{"shipped": {case: [weights, rgb, depth, alphas, invalid], "rerun": bool}, "plain": the same of the build without the loop}"""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    variant = os.path.join(ROOT, "behindthescenes_amd", "variants", "libbts_nosharedtexels.so")
    assert os.path.exists(variant), f"{variant} missing: __graft_entry__.build() builds the variants"
    d = tmp_path_factory.mktemp("shared_texels")
    res = {}
    for tag, lib in (("shipped", None), ("plain", variant)):
        env = dict(os.environ)
        env.pop("BTS_RENDER_LIB", None)
        if lib:
            env["BTS_RENDER_LIB"], env["BTS_ALLOW_LIB_OVERRIDE"] = lib, "1"
        f = d / f"{tag}.pt"
        r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, hd=HD), str(f)], env=env, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = torch.load(f)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_shared_loop_matches_the_build_without_it(rendered, name):
    sh = shared_class(name)
    frac = sh.float().mean().item()
    print(f"{name}: {sh.numel()} rays, shared class {frac:.3f}")
    assert frac >= 0.25, f"{name}: only {frac:.3f} of the rays share their texels: the case does not exercise the shared loop"
    assert 1.0 - frac >= 0.25, f"{name}: only {1.0 - frac:.3f} of the rays do not share their texels: the loops never alternate"
    for what, a, b in zip(NAMES, rendered["shipped"][name], rendered["plain"][name]):
        assert torch.isfinite(a).all(), what
        assert torch.equal(a, b), f"{name}: {what}: {(a != b).sum().item()} of {a.numel()} values differ from the build without the shared loop"


@pytest.mark.gpu
def test_shared_loop_rerun(rendered):
    """20 launches of eval_like: every output identical to the first (the image's LDS-DMA write against the previous ray's reads)."""
    assert rendered["shipped"]["rerun"] is True
    assert rendered["plain"]["rerun"] is True


@pytest.mark.parametrize("name", ["eval_like", "near_miss"])
def test_cases_hold_both_classes(name):
    """No GPU: the input condition (both classes are there before anything is rendered), for the flagship's structure and for the
    case whose shift was chosen for it."""
    frac = shared_class(name).float().mean().item()
    assert 0.25 <= frac <= 0.75, (name, frac)
