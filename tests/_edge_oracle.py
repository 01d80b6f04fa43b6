"""Plain torch restatements of the kernels at the two ends of the render path (csrc/bts_aux.hip) with the working precision as a
parameter: ray generation (util.py:113-149, 244-273), stratified depth sampling (nerf.py:103-123), distance -> z
(projection_operations.py:4-16), the rgb0 packing of encode's ``images * .5 + .5`` (models_bts.py:82) and PatchRaySampler.sample
(ray_sampler.py:125-162) as a gather.  In torch.float32 every function is oracle.bts_oracle's statement operation by operation
(tests/test_edge_oracle_cpu.py holds them bit for bit); in torch.float64 it is the same formulas and nothing else -- the yardstick the
bars of tests/test_gpu_edge_kernels.py are measured from.  The inputs stay the fp32 values the kernels read; only the arithmetic changes."""
import torch


def gen_rays(poses_c2w, projs, H, W, z_near, z_far, norm_dir=True, dtype=torch.float32, near_far=None):
    """poses (V, 4, 4), projs (V, 3, 3) -> rays (V, H, W, 8) = [c2w translation, R @ unproj(pixel), near, far].  The pixel grid is
    linspace(-1, 1, W) x linspace(-1, 1, H) formed in ``dtype``; ``near_far`` (V, 2): the planes per view (gen_rays_nf) instead of
    z_near / z_far."""
    V = poses_c2w.shape[0]
    poses, projs = poses_c2w.to(dtype), projs.to(dtype)
    focal, center = projs[:, [0, 1], [0, 1]], projs[:, [0, 1], [2, 2]]
    gx = torch.linspace(-1, 1, W, dtype=dtype).view(1, 1, W).expand(V, H, W)
    gy = torch.linspace(-1, 1, H, dtype=dtype).view(1, H, 1).expand(V, H, W)
    g = torch.stack((gx, gy), dim=-1)
    g = (g - center.view(V, 1, 1, 2)) / focal.view(V, 1, 1, 2)
    d = torch.cat((g, torch.ones_like(gx).unsqueeze(-1)), dim=-1)
    if norm_dir:
        d = d / torch.norm(d, dim=-1).unsqueeze(-1)
    origins = poses[:, None, None, :3, 3].expand(-1, H, W, -1)
    d_world = torch.matmul(poses[:, None, None, :3, :3], d.unsqueeze(-1))[..., 0]
    if near_far is None:
        near = torch.full((V, H, W, 1), float(z_near), dtype=dtype)
        far = torch.full((V, H, W, 1), float(z_far), dtype=dtype)
    else:
        nf = near_far.to(dtype)
        near, far = nf[:, 0].view(V, 1, 1, 1).expand(V, H, W, 1), nf[:, 1].view(V, 1, 1, 1).expand(V, H, W, 1)
    return torch.cat((origins, d_world, near, far), dim=-1)


def image_rays(poses_c2w, projs, H, W, z_near, z_far, norm_dir=True, dtype=torch.float32):
    """poses (n, v, 4, 4), projs (n, v, 3, 3) -> the full ray volume (n, v, H, W, 8)"""
    return torch.stack([gen_rays(poses_c2w[i], projs[i], H, W, z_near, z_far, norm_dir, dtype) for i in range(poses_c2w.shape[0])])


def sample_coarse(rays, u, lindisp, dtype=torch.float32):
    """rays (B, 8) with near / far per ray in columns 6 and 7, u (B, K) in [0, 1) -> z (B, K): s_k = linspace(0, 1 - 1/K, K)[k] + u / K,
    then depth-linear or disparity-linear between near and far."""
    B, K = u.shape
    near, far = rays[:, 6:7].to(dtype), rays[:, 7:8].to(dtype)
    step = 1.0 / K
    s = torch.linspace(0, 1 - step, K, dtype=dtype).unsqueeze(0).repeat(B, 1)
    s = s + u.to(dtype) * step
    if not lindisp:
        return near * (1 - s) + far * s
    return 1 / (1 / near * (1 - s) + 1 / far * s)


def distance_to_z(depths, projs, dtype=torch.float32):
    """depths (n, nv, H, W), projs (n, nv, 3, 3) -> z = depth * cam.z / |cam|, cam = inv(K) @ [gx, gy, 1]; the inverse of the fp32
    intrinsics is taken in ``dtype``."""
    n, nv, h, w = depths.shape
    inv_K = torch.inverse(projs.to(dtype))
    gx = torch.linspace(-1, 1, w, dtype=dtype).view(1, 1, 1, -1).expand(-1, -1, h, -1)
    gy = torch.linspace(-1, 1, h, dtype=dtype).view(1, 1, -1, 1).expand(-1, -1, -1, w)
    pix = torch.stack((gx, gy, torch.ones_like(gx)), dim=2).expand(n, nv, -1, -1, -1)
    cam = (inv_K @ pix.reshape(n, nv, 3, -1)).view(n, nv, 3, h, w)
    return depths.to(dtype) * (cam[:, :, 2] / torch.norm(cam, dim=2))


def pack_rgb(images, scale, shift, dtype=torch.float32):
    """(..., 3, H, W) -> (..., H, W, 4) rgb0: multiply, then add, each rounded to ``dtype``; the fourth channel is 0"""
    x = images.to(dtype)
    x = (x * torch.tensor(scale, dtype=dtype)) + torch.tensor(shift, dtype=dtype)
    x = x.movedim(-3, -1)
    return torch.cat((x, torch.zeros_like(x[..., :1])), dim=-1).contiguous()


def patch_rays(ray_volume, images, patch_v, patch_y, patch_x, ph, pw):
    """PatchRaySampler.sample as a gather: ray_volume (n, v, H, W, 8), images (n, v, c, H, W) | None, patch_* (n, P) integers ->
    rays (n, P * ph * pw, 8), colours (n, P * ph * pw, c) | None, patch-major, then row, then column."""
    (n, P), dev = patch_v.shape, ray_volume.device
    smp = torch.arange(n, device=dev).view(n, 1, 1, 1)
    view = patch_v.long().to(dev).view(n, P, 1, 1)
    y = patch_y.long().to(dev).view(n, P, 1, 1) + torch.arange(ph, device=dev).view(1, 1, ph, 1)
    x = patch_x.long().to(dev).view(n, P, 1, 1) + torch.arange(pw, device=dev).view(1, 1, 1, pw)
    rays = ray_volume[smp, view, y, x].reshape(n, P * ph * pw, 8)
    gt = None if images is None else images[smp, view, :, y, x].reshape(n, P * ph * pw, images.shape[2])
    return rays, gt


def random_rotations(count, gen):
    """uniformly random rotations (count, 3, 3) in fp64: the Q of a Gaussian matrix with R's diagonal made positive, det +1"""
    q, r = torch.linalg.qr(torch.randn(count, 3, 3, generator=gen, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1)).unsqueeze(-2)
    return q * torch.sign(torch.linalg.det(q)).view(count, 1, 1)


def random_poses(count, gen, spread=50.0):
    """rigid c2w poses (count, 4, 4) in fp32: uniformly random rotations, translations of order ``spread``"""
    m = torch.zeros(count, 4, 4, dtype=torch.float64)
    m[:, :3, :3], m[:, :3, 3], m[:, 3, 3] = random_rotations(count, gen), spread * torch.randn(count, 3, generator=gen, dtype=torch.float64), 1.0
    return m.float()


def random_intrinsics(count, gen):
    """per-view intrinsics (count, 3, 3) in normalised units with fx != fy and an off-centre principal point"""
    r = torch.rand(count, 4, generator=gen)
    K = torch.zeros(count, 3, 3)
    K[:, 0, 0], K[:, 1, 1] = 0.7 + 0.9 * r[:, 0], 1.5 + 2.5 * r[:, 1]
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 0.5 * r[:, 2] - 0.25, 0.4 * r[:, 3] - 0.2, 1.0
    return K


# ---- the small inverse ---------------------------------------------------------------------------------------------------------------
INVERSE_FAMILIES = ("rigid", "permuted", "K_normalised", "K_pixels", "random")


def _axis_rotations(count, gen, angle):
    """rotations within ``angle`` radians of the identity (angle = 0: the identity itself), fp64"""
    w = angle * (2 * torch.rand(count, 3, generator=gen, dtype=torch.float64) - 1)
    S = torch.zeros(count, 3, 3, dtype=torch.float64)
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 2] = -w[:, 2], w[:, 1], -w[:, 0]
    return torch.linalg.matrix_exp(S - S.transpose(-1, -2))


def inverse_family(family, d, N, gen):
    """fp32 matrices (N, d, d) of one family of tests/test_gpu_edge_kernels.py:
        rigid         c2w poses, uniformly random rotations, translations of order 50 (d = 3: the rotation alone)
        permuted      poses with their rows moved round by one.  In turn: a uniformly random rotation; a rotation within 0.2 rad of the
                      identity; the identity itself (an axis-permuting pose, as KITTI's velodyne-to-camera ones: exact zeros on the
                      diagonal).  In the last two the largest entry of EVERY column sits off the diagonal: every column needs the swap
        K_normalised  intrinsics in normalised units          K_pixels  in pixel units (fx about 550, cx about 680)
        random        singular values from 1 down to 1 / 800: condition number at most 1e3"""
    if family in ("rigid", "permuted"):
        R = random_rotations(N, gen)
        if family == "permuted":
            near, which = _axis_rotations(N, gen, 0.2), torch.arange(N) % 3
            R = torch.where((which == 0).view(N, 1, 1), R, torch.where((which == 1).view(N, 1, 1), near, torch.eye(3, dtype=torch.float64).expand(N, 3, 3)))
            R = torch.roll(R, 1, dims=1)
        m = torch.zeros(N, 4, 4, dtype=torch.float64)
        m[:, :3, :3], m[:, :3, 3], m[:, 3, 3] = R, 50.0 * torch.randn(N, 3, generator=gen, dtype=torch.float64), 1.0
        return m[:, :d, :d].float().contiguous()
    if family in ("K_normalised", "K_pixels"):
        K = random_intrinsics(N, gen)
        if family == "K_pixels":
            r = torch.rand(N, 4, generator=gen)
            K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 500 + 100 * r[:, 0], 520 + 100 * r[:, 1], 640 + 80 * r[:, 2], 170 + 40 * r[:, 3]
        if d == 3:
            return K
        m = torch.eye(4).repeat(N, 1, 1)
        m[:, :3, :3] = K
        return m
    assert family == "random", family
    u, _ = torch.linalg.qr(torch.randn(N, d, d, generator=gen, dtype=torch.float64))
    v, _ = torch.linalg.qr(torch.randn(N, d, d, generator=gen, dtype=torch.float64))
    s = torch.exp(-6.68 * torch.rand(N, d, generator=gen, dtype=torch.float64))
    s[:, 0] = 1.0
    return ((u * s.unsqueeze(-2)) @ v.transpose(-1, -2)).float()


def inverse_excess(got, m):
    """By how much ``got`` (..., d, d) leaves |got - ref| <= 2^-23 |ref| + 1e-10 max|ref|, ref = torch.linalg.inv of the same fp32 entries
    in fp64 (<= 0: inside, entrywise).  The first term is one rounding to fp32; the second covers an fp64 elimination at condition
    numbers up to 1e3 (about 1e-13 max|ref|) with orders of magnitude to spare."""
    ref = torch.linalg.inv(m.double())
    top = ref.abs().amax(dim=(-1, -2), keepdim=True)
    return float(((got.double() - ref).abs() - (2.0 ** -23 * ref.abs() + 1e-10 * top)).max())
