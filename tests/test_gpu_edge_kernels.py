"""GPU: the kernels at the two ends of the render path (csrc/bts_aux.hip) -- layout changes, rgb0 packing, ray generation, patch rays,
stratified depths, distance -> z, the small inverse -- at every regime of their loops and at their edges.  Every element of every
output is asserted; there is no mask.  Three instruments:

  exact         wherever the operation is exact or exact per operation (-ffp-contract=off: x * scale + shift must be torch's bits):
                both transposes, pack_rgb, ray origins, near / far, the gathered colours, patch_rays against slices of gen_rays.
  trip / trip   a call that needs a second trip of its grid-stride loop must be bit-equal to the same entry point called on pieces
                that each fit one trip (per view, per frame, per block of rays): any index slip past the first trip shows.
                One trip: pack_rgb 2048 x 1024 pixels; gen_rays, gen_rays_nf, distance_to_z 2048 x 256; patch_rays, sample_coarse
                4096 x 256 (the launch functions).
  fp64 bar      directions, depths and z: at most 2 * D from tests/_edge_oracle.py's fp64 restatement in the sup norm, D the fp32
                oracle's (oracle.bts_oracle) own distance from it on the same inputs, computed here -- absolute for directions,
                relative for depths and z.
The inverse is held entrywise to |got - ref| <= 2^-23 |ref| + 1e-10 max|ref| against torch.linalg.inv of the same entries in fp64:
the first term is the one rounding to fp32 the kernel claims, the second covers an fp64 elimination at condition numbers up to 1e3
with orders of magnitude to spare.  Derived, not measured.
Ragged ends are run through the library entry on a buffer with a sentinel tail that must stay untouched.

Measured on MI355X, the kernel's distance from fp64 | D of the fp32 oracle on the same inputs (the bar is 2 * D):
    gen_rays (V x H x W), directions, absolute     norm_dir on                 norm_dir off
        1 x 1 x 1                                  4.665e-08 | 4.665e-08       3.067e-08 | 3.067e-08
        2 x 1 x 7                                  1.069e-07 | 1.069e-07       5.800e-08 | 5.800e-08
        2 x 5 x 1                                  7.158e-08 | 9.360e-08       1.435e-07 | 1.435e-07
        3 x 7 x 333                                1.467e-07 | 1.554e-07       1.507e-07 | 1.787e-07
        5 x 192 x 640 (two trips)                  1.649e-07 | 1.715e-07       2.713e-07 | 2.739e-07
    sample_coarse (B = 333), depths, relative      disparity-linear            depth-linear
        K = 1                                      1.268e-07 | 1.268e-07       9.760e-08 | 9.760e-08
        K = 2                                      6.821e-07 | 6.821e-07       1.256e-07 | 1.256e-07
        K = 7                                      1.292e-06 | 1.292e-06       1.886e-07 | 1.886e-07
        K = 64                                     2.002e-06 | 2.002e-06       1.326e-07 | 1.326e-07
        K = 65                                     2.361e-06 | 2.361e-06       1.883e-07 | 1.883e-07
        K = 130                                    5.126e-06 | 5.126e-06       2.082e-07 | 2.082e-07
        K = 256                                    3.843e-06 | 3.843e-06       1.440e-07 | 1.440e-07
        B = 16 400, K = 64 (two trips)             4.300e-06 | 4.300e-06       1.635e-07 | 1.635e-07
    distance_to_z (n x nv x H x W), z, relative
        1 x 1 x 1 x 1      1.023e-07 | 1.023e-07        1 x 2 x 1 x 9      7.830e-08 | 1.228e-07
        1 x 2 x 6 x 1      1.018e-07 | 1.018e-07        1 x 2 x 7 x 333    1.395e-07 | 1.395e-07
        1 x 5 x 192 x 640 (two trips)                   2.286e-07 | 2.286e-07
(The kernels do the oracle's fp32 operations, so most distances are the oracle's own; gen_rays differs where its R @ d is a chain of
fused multiply-adds and torch's matmul is not, distance_to_z where its inverse is rounded once from fp64 and torch.inverse is an fp32 LU.)
Everything exact and every trip / trip comparison was bit-equal; every inverse was inside its bound.
"""
import ctypes as C

import pytest
import torch

from oracle import bts_oracle as O
from tests import _edge_oracle as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL, SENTINEL = 4096, -7.0
Z_NEAR, Z_FAR = 2.7, 83.1            # (not representable: the planes must arrive as the fp32 values of these)


@pytest.fixture(scope="module")
def hip():
    import behindthescenes_amd as bts
    from behindthescenes_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return bts


def gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * 1009 ** i for i, s in enumerate(seed)) % (2 ** 31))


def call(name, *args):
    """the library entry itself, on the current stream"""
    from behindthescenes_amd import _lib
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(getattr(_lib.load(), name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], stream), name)


def tailed(count):
    return torch.full((count + TAIL,), SENTINEL, device=DEV)


def body(buf, *shape):
    count = 1
    for s in shape:
        count *= s
    assert buf.numel() == count + TAIL and bool((buf[count:] == SENTINEL).all()), "a store behind the end of the output"
    return buf[:count].view(*shape)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


# ---- transposes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 1, 3, 5), (1, 65, 1, 64), (2, 130, 5, 13), (1, 103, 7, 19), (1, 64, 64, 65)])
def test_transposes_past_one_channel_tile_and_at_the_smallest_sizes(hip, shape):
    """blockIdx.y >= 1 (C = 65, 103, 130), C = 1, HW < 64, HW = 64 * 65; every call on a buffer with a sentinel tail"""
    from behindthescenes_amd import native
    N, Cc, H, W = shape
    x = torch.randn(*shape, generator=gen(*shape)).to(DEV)
    want = x.permute(0, 2, 3, 1).contiguous()
    buf = tailed(x.numel())
    call("bts_nchw_to_nhwc", x, buf, N, Cc, H, W)
    y = body(buf, N, H, W, Cc)
    assert same(y, want) and same(native.nchw_to_nhwc(x), want)
    back = tailed(x.numel())
    call("bts_nhwc_to_nchw", want, back, N, Cc, H, W)
    assert same(body(back, N, Cc, H, W), x) and same(native.nhwc_to_nchw(want), x)


# ---- pack_rgb -----------------------------------------------------------------------------------------------------------------------
SCALES = [(0.5, 0.5), (0.3, 0.7)]          # exact products | inexact: a contracted multiply-add would give other bits


def frames(N, H, W, seed):
    return torch.rand(N, 3, H, W, generator=gen(N, H, W, seed)) * 2 - 1


@pytest.mark.parametrize("scale,shift", SCALES)
@pytest.mark.parametrize("total", [1, 255, 768, 769, 1023, 1024, 1025])
def test_pack_rgb_where_a_work_group_splits_between_its_two_loops(hip, total, scale, shift):
    """a thread takes the four-pixel loop while i0 + 768 < total: at 769 .. 1024 the threads of ONE work-group split between it and the
    ragged loop, at 768 none takes it, at 1025 a second work-group has one pixel"""
    im = frames(1, 1, total, 0)
    buf = tailed(total * 4)
    call("bts_pack_rgb", im.to(DEV), buf, 1, 1, total, C.c_float(scale), C.c_float(shift))
    assert same(body(buf, 1, 1, total, 4).cpu(), E.pack_rgb(im, scale, shift))


@pytest.mark.parametrize("scale,shift", SCALES)
def test_pack_rgb_with_one_threads_pixels_in_different_frames(hip, scale, shift):
    """(N, H, W) = (6, 11, 17): a frame is 187 pixels, a thread's four pixels are 256 apart"""
    from behindthescenes_amd import native
    im = frames(6, 11, 17, 1)
    want = E.pack_rgb(im, scale, shift)
    buf = tailed(6 * 11 * 17 * 4)
    call("bts_pack_rgb", im.to(DEV), buf, 6, 11, 17, C.c_float(scale), C.c_float(shift))
    assert same(body(buf, 6, 11, 17, 4).cpu(), want)
    assert same(native.pack_rgb(im.view(2, 3, 3, 11, 17).to(DEV), scale, shift).cpu(), want.view(2, 3, 11, 17, 4))
    assert not want[..., 3].any() and bool((want[..., :3] == (im * scale + shift).permute(0, 2, 3, 1)).all())


def test_pack_rgb_second_trip(hip):
    """17 x 193 x 641 = 2 103 121 pixels > 2048 x 1024: 5 969 pixels in a ragged second trip; against the frames packed one call each
    (one trip: 123 713 pixels) and against torch"""
    from behindthescenes_amd import native
    N, H, W = 17, 193, 641
    im = frames(N, H, W, 2)
    im_d = im.to(DEV)
    for scale, shift in SCALES:
        buf = tailed(N * H * W * 4)
        call("bts_pack_rgb", im_d, buf, N, H, W, C.c_float(scale), C.c_float(shift))
        got = body(buf, N, H, W, 4)
        pieces = torch.cat([native.pack_rgb(im_d[i:i + 1], scale, shift) for i in range(N)])
        assert same(got, pieces)
        assert same(got.cpu(), E.pack_rgb(im, scale, shift))


# ---- gen_rays -----------------------------------------------------------------------------------------------------------------------
RAY_SHAPES = [(1, 1, 1), (2, 1, 7), (2, 5, 1), (3, 7, 333), (5, 192, 640)]      # the last: 614 400 pixels > 2048 x 256
_RAYS = {}


def ray_case(V, H, W, norm_dir):
    """cameras of a case, the fp64 restatement of its rays and the fp32 oracle's distance D from it: computed once, left unchanged"""
    key = (V, H, W, bool(norm_dir))
    if key not in _RAYS:
        g = gen(V, H, W)
        poses, projs = E.random_poses(V, g), E.random_intrinsics(V, g)
        f64 = E.gen_rays(poses, projs, H, W, Z_NEAR, Z_FAR, norm_dir, torch.float64)
        o32 = O.gen_rays(poses, W, H, Z_NEAR, Z_FAR, projs[:, [0, 1], [0, 1]], projs[:, [0, 1], [2, 2]], norm_dir)
        D = float((o32[..., 3:6].double() - f64[..., 3:6]).abs().max())
        _RAYS[key] = dict(poses=poses, projs=projs, f64=f64, D=D)
    return _RAYS[key]


def lib_gen_rays(poses, projs, H, W, norm_dir):
    V = poses.shape[0]
    buf = tailed(V * H * W * 8)
    call("bts_gen_rays", poses, projs, V, H, W, C.c_float(Z_NEAR), C.c_float(Z_FAR), int(norm_dir), buf)
    return body(buf, V, H, W, 8)


@pytest.mark.parametrize("norm_dir", [True, False])
@pytest.mark.parametrize("V,H,W", RAY_SHAPES)
def test_gen_rays_at_the_edges_and_past_one_trip(hip, V, H, W, norm_dir):
    from behindthescenes_amd import native
    c = ray_case(V, H, W, norm_dir)
    poses, projs = c["poses"].to(DEV), c["projs"].to(DEV)
    got = lib_gen_rays(poses, projs, H, W, norm_dir)
    assert same(native.gen_rays(poses, projs, H, W, Z_NEAR, Z_FAR, norm_dir), got)
    # exact: origins and planes
    assert same(got[..., :3], poses[:, None, None, :3, 3].expand(V, H, W, 3).contiguous())
    assert bool((got[..., 6] == torch.tensor(Z_NEAR, device=DEV)).all()) and bool((got[..., 7] == torch.tensor(Z_FAR, device=DEV)).all())
    # trip against trip: one call per view
    if V > 1:
        assert same(got, torch.cat([native.gen_rays(poses[v:v + 1].contiguous(), projs[v:v + 1].contiguous(), H, W, Z_NEAR, Z_FAR, norm_dir)
                                    for v in range(V)]))
    # the fp64 bar on the directions, absolute
    dist = float((got[..., 3:6].cpu().double() - c["f64"][..., 3:6]).abs().max())
    print(f"gen_rays {V} x {H} x {W} norm_dir={int(norm_dir)}: {dist:.3e} | D {c['D']:.3e}")
    assert dist <= 2 * c["D"]


@pytest.fixture(scope="module")
def tiny_field(hip):
    """one encoded sample with one colour view: what a chunk of novel views renders from"""
    from tests._hip_helpers import build_net
    cfg = O.FieldConfig()
    scene = O.synthetic_scene(1, 1, 32, 64, 64, seed=0, smooth=True)
    mlp = O.init_mlp(64 + 39, 64, 0, gen=torch.Generator().manual_seed(0))
    net = build_net(cfg, mlp, scene, [0], device=DEV)
    net.set_scale(0)
    return net


@pytest.mark.parametrize("norm_dir", [True, False])
@pytest.mark.parametrize("V,H,W", [(2, 1, 7), (5, 192, 640)])
def test_gen_rays_nf_is_gen_rays_with_the_planes_per_view(hip, tiny_field, V, H, W, norm_dir):
    """gen_rays_nf_kernel runs inside bts_novel_views only: reached as novel_views.py reaches it, one chunk of V poses; the rays scratch
    of the call must hold gen_rays' origins and directions bit for bit and each view's own planes in columns 6 and 7"""
    from behindthescenes_amd import native
    c = ray_case(V, H, W, norm_dir)
    poses, projs = c["poses"].to(DEV), c["projs"].to(DEV)
    nf = torch.tensor([[0.5 + 1.25 * v, 20.3 + 17.0 * v] for v in range(V)])
    renderer = hip.NeRFRenderer(n_coarse=64, lindisp=True, hard_alpha_cap=True).to(DEV).eval()
    nv = hip.FusedNovelViews(renderer.bind_parallel(tiny_field), hip.ImageRaySampler(3.0, 80.0, H, W, norm_dir=norm_dir), poses_per_call=8)
    nv.render(poses, projs, nf.to(DEV))
    (rays,) = [sc["rays"] for sc in nv._scratch.values()]
    rays = rays.view(V, H, W, 8)
    # gen_rays one view at a time: calls of one trip each, held against fp64 by the test above
    want = torch.cat([native.gen_rays(poses[v:v + 1].contiguous(), projs[v:v + 1].contiguous(), H, W, Z_NEAR, Z_FAR, norm_dir) for v in range(V)])
    assert same(rays[..., :6], want[..., :6])
    assert same(rays[..., 6:].cpu(), nf.view(V, 1, 1, 2).expand(V, H, W, 2).contiguous())


# ---- patch_rays ---------------------------------------------------------------------------------------------------------------------
PN, PV, PH, PW = 2, 3, 24, 40          # samples, views and frame size of every patch case


def patch_scene(c, norm_dir=True):
    g = gen(7, c)
    poses, projs = E.random_poses(PN * PV, g).view(PN, PV, 4, 4).to(DEV), E.random_intrinsics(PN * PV, g).view(PN, PV, 3, 3).to(DEV)
    images = (torch.rand(PN, PV, c, PH, PW, generator=g) * 2 - 1).to(DEV)
    from behindthescenes_amd import native
    volume = torch.stack([native.gen_rays(poses[i].contiguous(), projs[i].contiguous(), PH, PW, Z_NEAR, Z_FAR, norm_dir) for i in range(PN)])
    return poses, projs, images, volume


def lib_patch_rays(poses, projs, images, c, pv, py, px, ph, pw, norm_dir=True):
    P = pv.shape[1]
    rays, gt = tailed(PN * P * ph * pw * 8), tailed(PN * P * ph * pw * c)
    call("bts_patch_rays", poses, projs, images, pv, py, px, PN, PV, c, PH, PW, P, ph, pw, C.c_float(Z_NEAR), C.c_float(Z_FAR), int(norm_dir),
         rays, gt)
    return body(rays, PN, P * ph * pw, 8), body(gt, PN, P * ph * pw, c)


def draws(P, ph, pw, g):
    """sample 0: random patches, with views 0 and v - 1 and the last legal position among them; sample 1: EVERY patch at y0 = H - ph,
    x0 = W - pw.  All inside the frame."""
    pv = torch.randint(0, PV, (PN, P), generator=g)
    py, px = torch.randint(0, PH - ph + 1, (PN, P), generator=g), torch.randint(0, PW - pw + 1, (PN, P), generator=g)
    pv[0, 0], pv[0, 1], py[0, 1], px[0, 1] = 0, PV - 1, PH - ph, PW - pw
    py[1], px[1], pv[1, 0], pv[1, 1] = PH - ph, PW - pw, PV - 1, 0
    assert 0 <= int(pv.min()) and int(pv.max()) < PV and 0 <= int(py.min()) and int(py.max()) + ph <= PH
    assert 0 <= int(px.min()) and int(px.max()) + pw <= PW
    return pv.int().to(DEV), py.int().to(DEV), px.int().to(DEV)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("ph,pw", [(1, 1), (3, 2), (8, 8), (1, 40), (24, 1)])
def test_patch_rays_are_slices_of_gen_rays_and_of_the_frames(hip, ph, pw, c):
    """(1, 40) and (24, 1): a patch as wide / as high as the frame, the only legal position is 0"""
    from behindthescenes_amd import native
    norm_dir = (ph, pw) != (3, 2)
    poses, projs, images, volume = patch_scene(c, norm_dir)
    pv, py, px = draws(7, ph, pw, gen(ph, pw, c))
    want_rays, want_gt = E.patch_rays(volume, images, pv, py, px, ph, pw)
    rays, gt = lib_patch_rays(poses, projs, images, c, pv, py, px, ph, pw, norm_dir)
    assert same(rays, want_rays) and same(gt, want_gt)
    n_rays, n_gt = native.patch_rays(poses, projs, images, pv, py, px, ph, pw, Z_NEAR, Z_FAR, norm_dir)
    assert same(n_rays, rays) and same(n_gt, gt)
    # the (H, W) tuple form: the same rays, no colours
    t_rays, t_gt = native.patch_rays(poses, projs, (PH, PW), pv, py, px, ph, pw, Z_NEAR, Z_FAR, norm_dir)
    assert t_gt is None and same(t_rays, rays)


def test_patch_rays_one_patch_64_wide(hip):
    """(ph, pw) = (1, 64) needs a frame at least 64 wide: 5 x 70"""
    from behindthescenes_amd import native
    g = gen(1, 64)
    n, v, H, W, P = 2, 2, 5, 70, 9
    poses, projs = E.random_poses(n * v, g).view(n, v, 4, 4).to(DEV), E.random_intrinsics(n * v, g).view(n, v, 3, 3).to(DEV)
    images = (torch.rand(n, v, 3, H, W, generator=g) * 2 - 1).to(DEV)
    volume = torch.stack([native.gen_rays(poses[i].contiguous(), projs[i].contiguous(), H, W, Z_NEAR, Z_FAR, True) for i in range(n)])
    pv, py, px = torch.randint(0, v, (n, P), generator=g), torch.randint(0, H, (n, P), generator=g), torch.randint(0, W - 64 + 1, (n, P), generator=g)
    py[1], px[1], pv[1, 0], pv[0, 0] = H - 1, W - 64, v - 1, 0
    assert int(py.max()) < H and int(px.max()) + 64 <= W and int(pv.max()) < v
    pv, py, px = pv.int().to(DEV), py.int().to(DEV), px.int().to(DEV)
    rays, gt = native.patch_rays(poses, projs, images, pv, py, px, 1, 64, Z_NEAR, Z_FAR)
    want_rays, want_gt = E.patch_rays(volume, images, pv, py, px, 1, 64)
    assert same(rays, want_rays) and same(gt, want_gt)


def test_patch_rays_second_trip(hip):
    """n = 2, P = 8200 patches of 8 x 8: 1 049 600 rays > 4096 x 256 (1024 in a second trip); against four blocks of 2050 patches,
    one call each, and against the slices"""
    from behindthescenes_amd import native
    poses, projs, images, volume = patch_scene(3)
    P = 8200
    pv, py, px = draws(P, 8, 8, gen(8200))
    rays, gt = lib_patch_rays(poses, projs, images, 3, pv, py, px, 8, 8)
    blocks = [native.patch_rays(poses, projs, images, pv[:, a:a + 2050].contiguous(), py[:, a:a + 2050].contiguous(),
                                px[:, a:a + 2050].contiguous(), 8, 8, Z_NEAR, Z_FAR) for a in range(0, P, 2050)]
    assert same(rays, torch.cat([b[0] for b in blocks], dim=1)) and same(gt, torch.cat([b[1] for b in blocks], dim=1))
    want_rays, want_gt = E.patch_rays(volume, images, pv, py, px, 8, 8)
    assert same(rays, want_rays) and same(gt, want_gt)


# ---- sample_coarse ------------------------------------------------------------------------------------------------------------------
def coarse_case(B, K, seed):
    g = gen(B, K, seed)
    rays = torch.randn(B, 8, generator=g)
    rays[:, 6] = 0.5 + 5.0 * torch.rand(B, generator=g)
    rays[:, 7] = rays[:, 6] + 10.0 + 90.0 * torch.rand(B, generator=g)
    return rays, torch.rand(B, K, generator=g)


def lib_sample_coarse(rays, u, lindisp):
    B, K = u.shape
    buf = tailed(B * K)
    call("bts_sample_coarse", rays, u, C.c_int64(B), K, int(lindisp), buf)
    return body(buf, B, K)


def rel_dist(a, ref64):
    return float(((a.double() - ref64).abs() / ref64.abs()).max())


def check_coarse(rays, u, lindisp, got, what):
    from behindthescenes_amd import native
    assert same(native.sample_coarse(rays.to(DEV), u.to(DEV), lindisp), got)
    got = got.cpu()
    f64 = E.sample_coarse(rays, u, lindisp, torch.float64)
    D = rel_dist(O.sample_coarse(rays, u.shape[1], lindisp, u), f64)
    dist = rel_dist(got, f64)
    print(f"sample_coarse {what} lindisp={int(lindisp)}: {dist:.3e} | D {D:.3e}")
    assert bool((got[:, 1:] >= got[:, :-1]).all())            # depths ascend along every ray
    assert dist <= 2 * D


@pytest.mark.parametrize("lindisp", [True, False])
@pytest.mark.parametrize("K", [1, 2, 7, 64, 65, 130, 256])
def test_sample_coarse_with_the_planes_of_every_ray(hip, K, lindisp):
    """near in [0.5, 5.5], far = near + [10, 100] per ray; B = 333 is ragged against every K here and more than one work-group"""
    rays, u = coarse_case(333, K, 0)
    check_coarse(rays, u, lindisp, lib_sample_coarse(rays.to(DEV), u.to(DEV), lindisp), f"B=333 K={K}")


@pytest.mark.parametrize("lindisp", [True, False])
def test_sample_coarse_second_trip(hip, lindisp):
    """B = 16 400, K = 64: 1 049 600 samples > 4096 x 256; against two blocks of 8200 rays"""
    from behindthescenes_amd import native
    rays, u = coarse_case(16400, 64, 1)
    rd, ud = rays.to(DEV), u.to(DEV)
    got = lib_sample_coarse(rd, ud, lindisp)
    assert same(got, torch.cat([native.sample_coarse(rd[a:a + 8200].contiguous(), ud[a:a + 8200].contiguous(), lindisp) for a in (0, 8200)]))
    check_coarse(rays, u, lindisp, got, "B=16400 K=64")


# ---- distance_to_z ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nv,H,W", [(1, 1, 1, 1), (1, 2, 1, 9), (1, 2, 6, 1), (1, 2, 7, 333), (1, 5, 192, 640)])
def test_distance_to_z_at_the_edges_and_past_one_trip(hip, n, nv, H, W):
    """depths from 1e-3 to 1e3 with a 0 and an inf among them (the single-pixel case has room for neither), anisotropic off-centre
    intrinsics per view; the last case is 614 400 pixels > 2048 x 256, against one call per view"""
    from behindthescenes_amd import native
    g = gen(n, nv, H, W)
    depths = torch.exp(torch.empty(n, nv, H, W).uniform_(-6.9, 6.9, generator=g))
    if depths.numel() >= 4:             # (not at the first or the last pixel: those keep a value that shows what was computed for them)
        depths.view(-1)[1], depths.view(-1)[depths.numel() // 2] = 0.0, float("inf")
    projs = E.random_intrinsics(n * nv, g).view(n, nv, 3, 3)
    d_d, K_d = depths.to(DEV), projs.to(DEV)
    inv_K = native.invert_small(K_d)
    buf = tailed(depths.numel())
    call("bts_distance_to_z", d_d, inv_K, n * nv, H, W, buf)
    got = body(buf, n, nv, H, W)
    assert same(hip.distance_to_z(d_d, K_d), got)
    if nv > 1:
        assert same(got, torch.cat([native.distance_to_z(d_d[:, v:v + 1].contiguous(), K_d[:, v:v + 1].contiguous()) for v in range(nv)], dim=1))
    got = got.cpu()
    f64, o32 = E.distance_to_z(depths, projs, torch.float64), O.distance_to_z(depths, projs)
    plain = torch.isfinite(depths) & (depths > 0)
    assert same(got[~plain], f64[~plain].float()) and int((~plain).sum()) == (2 if depths.numel() >= 4 else 0)      # 0 -> 0, inf -> inf
    D, dist = rel_dist(o32[plain], f64[plain]), rel_dist(got[plain], f64[plain])
    print(f"distance_to_z {n} x {nv} x {H} x {W}: {dist:.3e} | D {D:.3e}")
    assert dist <= 2 * D


# ---- invert_small -------------------------------------------------------------------------------------------------------------------
FAMILIES = list(E.INVERSE_FAMILIES)
matrices = E.inverse_family


def check_inverse(got, m):
    assert got.shape == m.shape and got.dtype == torch.float32
    excess = E.inverse_excess(got, m)
    assert excess <= 0.0, excess


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d", [3, 4])
def test_invert_small_is_the_fp64_inverse_rounded_once(hip, d, family):
    """N = 1, 63, 64, 65, 200 (a ragged work-group, exactly one, a second one), a (2, 3, d, d) batch shape and a non-contiguous input"""
    from behindthescenes_amd import native
    g = gen(d, FAMILIES.index(family))
    for N in (1, 63, 64, 65, 200):
        m = matrices(family, d, N, g)
        if family == "random":
            assert float(torch.linalg.cond(m.double()).max()) <= 1e3
        buf = tailed(N * d * d)
        call("bts_invert_small", m.to(DEV), buf, N, d)
        got = body(buf, N, d, d)
        assert same(native.invert_small(m.to(DEV)), got)
        check_inverse(got.cpu(), m)
    m = matrices(family, d, 6, g)
    check_inverse(native.invert_small(m.view(2, 3, d, d).to(DEV)).cpu(), m.view(2, 3, d, d))
    t = m.to(DEV).transpose(-1, -2)
    assert not t.is_contiguous()
    check_inverse(native.invert_small(t).cpu(), m.transpose(-1, -2))


@pytest.mark.parametrize("d", [3, 4])
def test_invert_small_singular_matrix_among_good_ones(hip, d):
    """exactly singular (two equal rows of small integers: the elimination reaches an exact 0 pivot): its own output is non-finite, the
    other matrices' bits are what they are without it"""
    from behindthescenes_amd import native
    m = matrices("rigid", d, 70, gen(5, d))
    clean = native.invert_small(m.to(DEV))
    bad = m.clone()
    s = torch.eye(d)
    s[:3, :3] = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 1.0, 4.0]])
    bad[37] = s
    got = native.invert_small(bad.to(DEV))
    assert not bool(torch.isfinite(got[37]).all())
    keep = torch.arange(70, device=DEV) != 37
    assert same(got[keep], clean[keep]) and bool(torch.isfinite(got[keep]).all())
