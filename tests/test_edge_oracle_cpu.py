"""CPU: tests/_edge_oracle.py in torch.float32 is oracle.bts_oracle's gen_rays / image_rays / sample_coarse / distance_to_z bit for bit --
on tests/golden/misc.npz's inputs, on shapes with H == 1 and with W == 1 and on the varied cameras and planes the GPU tests use.  Its
torch.float64 form, the yardstick of tests/test_gpu_edge_kernels.py, is then the same formulas and nothing else.  The gather form of
PatchRaySampler.sample is held against the reference's loop over patches (slices of the oracle's ray volume) and the golden fixture's
colours, pack_rgb against the two roundings taken from exact fp64 products, and the out-of-frame check of
``PatchRaySampler.sample(patches=...)`` -- host code -- is asserted here on CPU tensors."""
import os

import numpy as np
import pytest
import torch

from oracle import bts_oracle as O
from tests import _edge_oracle as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(12, 20), (1, 7), (5, 1), (1, 1), (7, 33)]        # misc.npz's size, H == 1, W == 1, both, an odd one


@pytest.fixture(scope="module")
def misc():
    z = np.load(os.path.join(GOLDEN, "misc.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def cameras(misc, varied):
    if not varied:
        return misc["poses"], misc["projs"]
    g = torch.Generator().manual_seed(3)
    V = misc["poses"].shape[0]
    return E.random_poses(V, g), E.random_intrinsics(V, g)


def oracle_rays(poses, projs, H, W, zn, zf, norm_dir):
    return O.gen_rays(poses, W, H, zn, zf, projs[:, [0, 1], [0, 1]], projs[:, [0, 1], [2, 2]], norm_dir)


@pytest.mark.parametrize("varied", [False, True])
@pytest.mark.parametrize("norm_dir", [True, False])
@pytest.mark.parametrize("H,W", SHAPES)
def test_gen_rays_in_fp32_is_the_oracle_bit_for_bit(misc, H, W, norm_dir, varied):
    poses, projs = cameras(misc, varied)
    want = oracle_rays(poses, projs, H, W, 3.0, 80.0, norm_dir)
    got = E.gen_rays(poses, projs, H, W, 3.0, 80.0, norm_dir)
    assert got.dtype == torch.float32 and got.shape == (poses.shape[0], H, W, 8) and torch.equal(got, want)
    # the batched form against image_rays
    P2, K2 = torch.stack((poses, poses.flip(0))), torch.stack((projs, projs.flip(0)))
    assert torch.equal(E.image_rays(P2, K2, H, W, 3.0, 80.0, norm_dir).reshape(2, -1, 8), O.image_rays(P2, K2, H, W, 3.0, 80.0, norm_dir))
    # per-view planes change columns 6 and 7 only
    nf = torch.tensor([[0.5 + i, 20.0 + 3 * i] for i in range(poses.shape[0])])
    per_view = E.gen_rays(poses, projs, H, W, 0.0, 0.0, norm_dir, near_far=nf)
    assert torch.equal(per_view[..., :6], want[..., :6])
    assert torch.equal(per_view[..., 6:], nf.view(-1, 1, 1, 2).expand(-1, H, W, 2))
    # fp64: the same inputs, a result of the other precision that the fp32 one rounds to within a few ulps
    f64 = E.gen_rays(poses, projs, H, W, 3.0, 80.0, norm_dir, torch.float64)
    assert f64.dtype == torch.float64 and torch.equal(f64[..., [0, 1, 2, 6, 7]].float(), want[..., [0, 1, 2, 6, 7]])
    assert float((f64[..., 3:6] - want[..., 3:6].double()).abs().max()) <= 2e-6


def test_gen_rays_on_the_golden_fixture(misc):
    """misc.npz's rays are the real reference's: the restatement is as close to them as the oracle is (the GPU test's 2e-6)"""
    for key, nd in (("rays_norm", True), ("rays_unnorm", False)):
        got = E.gen_rays(misc["poses"], misc["projs"], 12, 20, 3.0, 80.0, nd)
        assert float((got - misc[key]).abs().max()) <= 2e-6
        assert float((E.gen_rays(misc["poses"], misc["projs"], 12, 20, 3.0, 80.0, nd, torch.float64) - misc[key].double()).abs().max()) <= 2e-6


@pytest.mark.parametrize("lindisp", [True, False])
@pytest.mark.parametrize("K", [1, 2, 7, 64, 65, 130, 256])
def test_sample_coarse_in_fp32_is_the_oracle_bit_for_bit(misc, K, lindisp):
    g = torch.Generator().manual_seed(K)
    B = 37
    rays = misc["rays_norm"].reshape(-1, 8)[:B].clone()
    u = torch.rand(B, K, generator=g)
    assert torch.equal(E.sample_coarse(rays, u, lindisp), O.sample_coarse(rays, K, lindisp, u))        # the fixture's planes
    rays[:, 6] = 0.5 + 5.0 * torch.rand(B, generator=g)
    rays[:, 7] = rays[:, 6] + 10.0 + 90.0 * torch.rand(B, generator=g)
    want = O.sample_coarse(rays, K, lindisp, u)
    assert torch.equal(E.sample_coarse(rays, u, lindisp), want)                                       # per-ray planes
    f64 = E.sample_coarse(rays, u, lindisp, torch.float64)
    assert f64.dtype == torch.float64 and float(((f64 - want.double()).abs() / f64.abs()).max()) <= 2e-5


@pytest.mark.parametrize("H,W", SHAPES)
def test_distance_to_z_in_fp32_is_the_oracle_bit_for_bit(misc, H, W):
    depths, projs = misc["depths"], misc["projs2"]
    n, nv = depths.shape[:2]
    if (H, W) == tuple(depths.shape[-2:]):
        assert torch.equal(E.distance_to_z(depths, projs), O.distance_to_z(depths, projs))
        # the real reference's values, as closely as the GPU test asks of the kernel
        assert float(((E.distance_to_z(depths, projs) - misc["dist_to_z"]).abs() / misc["dist_to_z"].abs()).max()) <= 2e-6
    g = torch.Generator().manual_seed(H * 100 + W)
    d = torch.exp(torch.empty(n, nv, H, W).uniform_(-6.9, 6.9, generator=g))
    K = E.random_intrinsics(n * nv, g).view(n, nv, 3, 3)
    want = O.distance_to_z(d, K)
    assert torch.equal(E.distance_to_z(d, K), want)
    f64 = E.distance_to_z(d, K, torch.float64)
    assert f64.dtype == torch.float64 and float(((f64 - want.double()).abs() / f64.abs()).max()) <= 2e-6


def test_pack_rgb_is_two_roundings():
    g = torch.Generator().manual_seed(0)
    im = torch.rand(2, 3, 3, 5, 7, generator=g) * 2 - 1
    for scale, shift in ((0.5, 0.5), (0.3, 0.7)):
        got = E.pack_rgb(im, scale, shift)
        assert got.shape == (2, 3, 5, 7, 4) and got.dtype == torch.float32 and got.is_contiguous()
        assert torch.equal(got[..., :3], (im * scale + shift).permute(0, 1, 3, 4, 2)) and not got[..., 3].any()
        # a product of two fp32 values is exact in fp64, and so is the sum of its rounding and the shift at these magnitudes
        s32, t32 = torch.tensor(scale).double(), torch.tensor(shift).double()
        two = ((im.double() * s32).float().double() + t32).float()
        assert torch.equal(got[..., :3], two.permute(0, 1, 3, 4, 2))
    # 0.3 * x + 0.7 is inexact: a fused multiply-add would give other bits somewhere
    fused = (im.double() * torch.tensor(0.3).double() + torch.tensor(0.7).double()).float()
    assert not torch.equal(E.pack_rgb(im, 0.3, 0.7)[..., :3], fused.permute(0, 1, 3, 4, 2))


def reference_patch_loop(volume, images, pv, py, px, ph, pw):
    """ray_sampler.py:145-160: per sample and patch, slices of the full ray volume and of the frames"""
    rays, gt = [], []
    for i in range(pv.shape[0]):
        r_i, g_i = [], []
        for p in range(pv.shape[1]):
            v, y, x = int(pv[i, p]), int(py[i, p]), int(px[i, p])
            r_i.append(volume[i, v, y:y + ph, x:x + pw].reshape(-1, 8))
            g_i.append(images[i, v, :, y:y + ph, x:x + pw].permute(1, 2, 0).reshape(ph * pw, -1))
        rays.append(torch.cat(r_i)), gt.append(torch.cat(g_i))
    return torch.stack(rays), torch.stack(gt)


def test_patch_rays_gather_is_the_reference_loop(misc):
    import behindthescenes_amd as bts
    imgs = misc["patch_images"]
    n, v, c, h, w = imgs.shape
    P2, K2 = misc["poses"].unsqueeze(0).expand(n, -1, -1, -1), misc["projs"].unsqueeze(0).expand(n, -1, -1, -1)
    volume = O.image_rays(P2, K2, h, w, 3.0, 80.0).view(n, v, h, w, 8)
    assert torch.equal(E.image_rays(P2, K2, h, w, 3.0, 80.0), volume)
    # the reference's seeded draws (tests/test_gpu_parity.py): the golden colours exactly, the golden rays as closely as the oracle's
    ps = bts.PatchRaySampler(ray_batch_size=48, z_near=3.0, z_far=80.0, patch_size=4)
    torch.manual_seed(11)
    pv, py, px = ps.draw_patches(n, v, h, w)
    rays, gt = E.patch_rays(volume, imgs, pv, py, px, 4, 4)
    want_rays, want_gt = reference_patch_loop(volume, imgs, pv, py, px, 4, 4)
    assert torch.equal(rays, want_rays) and torch.equal(gt, want_gt)
    assert torch.equal(gt, misc["patch_rgb"]) and float((rays - misc["patch_rays"]).abs().max()) <= 2e-6
    # odd patch shapes, patches at the last legal row / column, one channel, no frames
    g = torch.Generator().manual_seed(1)
    for ph, pw in ((1, 1), (3, 2), (h, 1), (1, w)):
        pv = torch.randint(0, v, (n, 5), generator=g)
        py, px = torch.randint(0, h - ph + 1, (n, 5), generator=g), torch.randint(0, w - pw + 1, (n, 5), generator=g)
        py[:, 0], px[:, 0], pv[:, 0], pv[:, 1] = h - ph, w - pw, 0, v - 1
        rays, gt = E.patch_rays(volume, imgs[:, :, :1], pv.int(), py.int(), px.int(), ph, pw)
        want_rays, want_gt = reference_patch_loop(volume, imgs[:, :, :1], pv, py, px, ph, pw)
        assert rays.shape == (n, 5 * ph * pw, 8) and gt.shape == (n, 5 * ph * pw, 1)
        assert torch.equal(rays, want_rays) and torch.equal(gt, want_gt)
        assert E.patch_rays(volume, None, pv, py, px, ph, pw)[1] is None


def test_patch_sampler_rejects_out_of_frame_patches_on_the_host(misc):
    """PatchRaySampler.sample(patches=...) checks the coordinates before anything reaches the device: CPU tensors never get that far"""
    import behindthescenes_amd as bts
    imgs = misc["patch_images"]
    n, v, c, h, w = imgs.shape
    P2, K2 = misc["poses"].unsqueeze(0).expand(n, -1, -1, -1), misc["projs"].unsqueeze(0).expand(n, -1, -1, -1)
    ps = bts.PatchRaySampler(ray_batch_size=2 * 3 * 2, z_near=3.0, z_far=80.0, patch_size=(3, 2))
    ok = [torch.zeros(n, 2, dtype=torch.int64) for _ in range(3)]
    for which, bad, name in ((0, v, "view"), (0, -1, "view"), (1, h - 3 + 1, "y0"), (1, -1, "y0"), (2, w - 2 + 1, "x0"), (2, -1, "x0")):
        draws = [t.clone() for t in ok]
        draws[which][n - 1, 1] = bad
        with pytest.raises(ValueError, match=name):
            ps.sample(imgs, P2, K2, patches=tuple(draws))
    # the last legal row / column passes the check (and then fails only because the frames are not on the GPU)
    draws = [t.clone() for t in ok]
    draws[0][:], draws[1][:], draws[2][:] = v - 1, h - 3, w - 2
    with pytest.raises(bts.native.BtsNativeError):
        ps.sample(imgs, P2, K2, patches=tuple(draws))


@pytest.mark.parametrize("d", [3, 4])
def test_inverse_families_and_their_bound(d):
    """the correctly rounded fp64 inverse meets |got - ref| <= 2^-23 |ref| + 1e-10 max|ref| on every family; a perturbation of one fp32
    ulp and a half does not; and two thirds of the permuted poses have the largest entry of every column off the diagonal"""
    for family in E.INVERSE_FAMILIES:
        m = E.inverse_family(family, d, 200, torch.Generator().manual_seed(d))
        assert m.shape == (200, d, d) and m.dtype == torch.float32
        ref = torch.linalg.inv(m.double())
        assert E.inverse_excess(ref.float(), m) <= 0.0, family
        assert E.inverse_excess((ref * (1 + 3.0 * 2.0 ** -24)).float(), m) > 0.0, family
        if family == "random":
            assert float(torch.linalg.cond(m.double()).max()) <= 1e3
        if family == "permuted":
            R = m[:, :3, :3].abs()
            off = R.diagonal(dim1=-2, dim2=-1) < R.amax(dim=-2)
            assert bool(off[torch.arange(200) % 3 != 0].all())
            assert float(torch.linalg.det(m[:, :3, :3].double()).sub(1).abs().max()) < 1e-6          # still rotations
