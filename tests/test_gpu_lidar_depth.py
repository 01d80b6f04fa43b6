"""GPU: the LiDAR ground-truth depth map (behindthescenes_amd.lidar_depth, csrc/bts_lidar_depth.hip) against the golden of the REAL
reference (tests/golden/lidar_depth.npz: both KITTI ``load_depth`` functions, (1, 2) .. (24, 40), fp32 and fp64 P, eigen_depth) and
against the numpy oracle (tests/_lidar_depth_oracle.py).

On every golden case the set of non-zero pixels is the reference's and every value belongs to the reference's source point (the z that
compete in a pixel or key group differ by 1e-3 relative; a value must sit within 5e-4 of its source's).  How close it must sit:
  fp32 P: per value at most TWICE as far from the exact z (rational arithmetic on the stored P and point) as the fp32 reference's
          own value lies -- a value the reference has exactly must be exact here.
  fp64 P: 4 u S with u = 2^-53 and S = |P20 x| + |P21 y| + |P22 z| + |P23|: the a-priori bound of a four-term dot product evaluated
          with one rounding per term, the same for any summation order.
Measured (MI355X, gfx950; ``test_every_golden_case`` prints the figures per case): all 2 656 non-zero values of the 20 cases are BIT-EQUAL
to the reference's.  fp32: largest distance from the exact z 2.51 half-ulps of z (kitti_raw 24 x 40; the reference's own: 2.51), largest
distance / bar 0.500 in every case.  fp64: largest distance 2.52 u S (kitti_raw 24 x 40; the reference's own: 2.52) against the bar of 4 u S.

Where a test demands ``torch.equal`` with the CPU oracle, its inputs are dyadic numbers whose products and sums are exact in fp32, so
that neither side's summation order enters: what is compared is the rule set, the IEEE division and the rounding to the pixel."""
import os

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import native
from oracle import bts_oracle as O

from tests import _lidar_depth_oracle as LD
from tests._hip_helpers import build_net

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar_depth.npz")
DEV = "cuda:0"
NAMES = [f"{c}_{s}_{t}" for c in LD.CONVENTIONS for s in ("1x2", "2x2", "5x7", "24x40") for t in ("f32", "f64")] + \
        [f"kitti_raw_{s}_{t}_eigen" for s in ("5x7", "24x40") for t in ("f32", "f64")]
U64 = 2.0 ** -53


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def case_of(gold, name):
    return dict(points=gold[name + "_points"], P=gold[name + "_P"], depth=gold[name + "_depth"], src=gold[name + "_src"],
                z_hi=gold[name + "_z_hi"], z_lo=gold[name + "_z_lo"], size=tuple(gold[name + "_depth"].shape[1:]),
                convention="kitti_raw" if name.startswith("kitti_raw") else "kitti_360", eigen=name.endswith("_eigen"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_the_list_of_cases_is_the_goldens(gold):
    assert sorted(NAMES) == sorted(gold["names"].tolist())


@pytest.mark.parametrize("name", NAMES)
def test_every_golden_case(gold, name):
    c = case_of(gold, name)
    out = bts.load_depth(dev(c["points"]), dev(c["P"]), c["size"], c["convention"], c["eigen"])
    assert out.shape == (1,) + c["size"] and out.dtype == (torch.float32 if "_f32" in name else torch.float64)
    mine = out.cpu().numpy().astype(np.float64)[0]
    ref = c["depth"][0]
    assert np.array_equal(mine != 0, ref != 0), name
    occ = ref != 0
    hi, lo = c["z_hi"][occ], c["z_lo"][occ]
    d_mine, d_ref = np.abs((mine[occ] - hi) - lo), np.abs((ref[occ] - hi) - lo)
    assert (d_mine <= 5e-4 * np.abs(hi)).all(), name                       # the reference's source point
    if "_f32" in name:
        bar = 2 * d_ref
        unit, what = np.abs(hi) * 2.0 ** -24, "fp32 ulp-halves of z"
    else:
        P, pts = c["P"], c["points"][c["src"][occ]].astype(np.float64)
        S = np.abs(P[2, 0] * pts[:, 0]) + np.abs(P[2, 1] * pts[:, 1]) + np.abs(P[2, 2] * pts[:, 2]) + np.abs(P[2, 3])
        bar = 4 * U64 * S
        unit, what = U64 * S, "u S"
    print(f"{name}: {int(occ.sum())} values, {int((mine[occ] == ref[occ]).sum())} bit-equal to the reference; distance from the exact z in {what}: "
          f"this {np.max(d_mine / unit):.3f}, reference {np.max(d_ref / unit):.3f}; largest this / bar {np.max(d_mine / np.maximum(bar, 1e-300)):.3f}")
    assert (d_mine <= bar).all(), (name, float(np.max(d_mine / unit)), float(np.max(d_ref / unit)))


# ---- exact inputs: dyadic P and points, every product and sum exact in fp32
def exact_P(convention, dtype):
    if convention == "kitti_raw":
        return np.array([[4, -8, 0, 1.25], [2, 0, -8, 1.0], [1, 0, 0, 0.5]], dtype=dtype)
    return np.array([[0, -1, 0, 0.125], [0, 0, -1, -0.25], [1, 0, 0, 0.5]], dtype=dtype)


def exact_point(convention, size, xp, yp, u2):
    """the point that lands a quarter pixel inside (xp, yp) with z = u2 under exact_P"""
    H, W = size
    x = u2 - 0.5
    if convention == "kitti_raw":
        return [x, (4 * x + 1.25 - (xp + 1.25) * u2) / 8, (2 * x + 1 - (yp + 1.25) * u2) / 8, 1.0]
    px, py = 2 * (xp + 0.25) / W - 1, 2 * (yp + 0.25) / H - 1
    return [x, 0.125 - px * u2, -0.25 - py * u2, 1.0]


def exact_cloud(convention, size, n, seed, keep_off=()):
    """n dyadic points on both sides of the camera, in and out of frame, none in the pixels ``keep_off``"""
    rng = np.random.default_rng(seed)
    H, W = size
    pts = []
    while len(pts) < n:
        xp, yp = int(rng.integers(-2, W + 2)), int(rng.integers(-2, H + 2))
        if (xp, yp) in keep_off:
            continue
        u2 = float(rng.integers(-4, 256)) / 4 + 0.125      # a few behind the camera, a few in front of it with x < 0
        pts.append(exact_point(convention, size, xp, yp, u2))
    pts = np.array(pts, dtype=np.float64)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    return pts.astype(np.float32)


@pytest.mark.parametrize("convention", LD.CONVENTIONS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_more_than_one_grid_trip_and_the_order_across_the_border(convention, dtype):
    """700 points with the points pass capped at ONE work-group: three trips of 256.  Pixel R = (W - 1, 1) holds point 10 (trip 0), its
    key partner L = (0, 2) points 300 (trip 1, the nearer) and 600 (trip 2): R, the first, receives 300's z from the row below, L keeps
    600's.  With the cloud reversed L's first point comes first: L receives the minimum, R keeps its only point."""
    size = (4, 8)
    H, W = size
    R, L = (W - 1, 1), (0, 2)
    P = exact_P(convention, dtype)
    pts = exact_cloud(convention, size, 700, 3, keep_off=(R, L))
    pts[10], pts[300], pts[600] = exact_point(convention, size, *R, 9.0), exact_point(convention, size, *L, 5.0), exact_point(convention, size, *L, 6.0)
    for cloud, want_R, want_L in ((pts, 5.0, 6.0), (np.ascontiguousarray(pts[::-1]), 9.0, 5.0)):
        want = LD.load_depth(cloud, P, size, convention)
        assert want[0, R[1], R[0]] == want_R and want[0, L[1], L[0]] == want_L
        assert np.array_equal(want, LD.literal(cloud, P, size, convention)) and (want != 0).sum() > 20
        out = native.lidar_depth(dev(cloud), (0, 700), dev(P), size, convention, max_blocks=1)
        assert torch.equal(out.cpu(), torch.from_numpy(want))
        assert torch.equal(out, native.lidar_depth(dev(cloud), (0, 700), dev(P), size, convention))      # one trip: the same map


@pytest.mark.parametrize("convention", LD.CONVENTIONS)
def test_no_point_and_a_cloud_wholly_behind_the_camera_give_zeros(convention):
    size = (4, 8)
    P = dev(exact_P(convention, np.float32))
    out = bts.load_depth(torch.zeros(0, 4, device=DEV), P, size, convention)
    assert out.shape == (1, 4, 8) and not out.any()
    behind = exact_cloud(convention, size, 300, 4)
    behind[:, 0] = -np.abs(behind[:, 0]) - 1.0            # u2 = x + 0.5 < 0
    assert not bts.load_depth(dev(behind), P, size, convention).any()
    assert not LD.load_depth(behind, exact_P(convention, np.float32), size, convention).any()
    if convention == "kitti_360":      # (kitti_raw's front filter drops them all) some land in frame: it is the clamp that makes the zeros
        assert (LD.load_depth(behind, exact_P(convention, np.float32), size, convention, mutant="no_clamp") < 0).any()
    torch.cuda.synchronize()


def test_batch_equals_single_calls_and_the_workspace_is_reused(gold):
    a, b = case_of(gold, "kitti_360_24x40_f32"), case_of(gold, "kitti_360_5x7_f32")
    P, size = dev(a["P"]), a["size"]
    clouds = [a["points"], a["points"][:0], a["points"][::-1][:400], a["points"][100:101]]
    offsets = np.cumsum([0] + [len(c) for c in clouds])
    batch = bts.load_depth_batch(dev(np.concatenate(clouds)), offsets.tolist(), P, size, "kitti_360")
    assert batch.shape == (4, 1) + size and not batch[1].any() and int((batch[3] != 0).sum()) <= 1
    first = bts.load_depth(dev(clouds[0]), P, size, "kitti_360")
    small = bts.load_depth(dev(b["points"]), dev(b["P"]), b["size"], "kitti_360")             # another (H, W) on the same workspace
    assert np.array_equal(small.cpu().numpy().astype(np.float64) != 0, b["depth"] != 0)
    for f, cloud in enumerate(clouds):
        assert torch.equal(batch[f], bts.load_depth(dev(cloud), P, size, "kitti_360")), f
    assert torch.equal(batch[0], first)
    assert torch.equal(batch, bts.load_depth_batch(dev(np.concatenate(clouds)), torch.from_numpy(offsets), P, size, "kitti_360"))


@pytest.mark.parametrize("name", ["kitti_raw_24x40_f32_eigen", "kitti_360_24x40_f64"])
def test_reruns_are_bit_identical(gold, name):
    c = case_of(gold, name)
    pts, P = dev(c["points"]), dev(c["P"])
    first = bts.load_depth(pts, P, c["size"], c["convention"], c["eigen"])
    assert torch.equal(first, bts.load_depth(pts, P, c["size"], c["convention"], c["eigen"]))


@pytest.mark.parametrize("size", [(5, 1), (4096, 4096)])
def test_unsupported_sizes_return_the_error_and_write_nothing(size):
    pts, P = dev(exact_cloud("kitti_raw", (4, 8), 64, 5)), dev(exact_P("kitti_raw", np.float32))
    out = torch.full((1,) + size, 7.0, device=DEV)
    with pytest.raises(bts.BtsNativeError, match="BTS_E_UNSUPPORTED"):
        native.lidar_depth(pts, (0, 64), P, size, "kitti_raw", out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(bts.BtsNativeError, match="points"):
        bts.load_depth(pts[:, :3].contiguous(), P, (5, 7), "kitti_raw")
    with pytest.raises(ValueError, match="offsets"):
        bts.load_depth_batch(pts, (0, 70), P, (5, 7), "kitti_raw")


def test_frame_lidar_is_frame_on_the_map_of_load_depth():
    n, v, H, W, C, K = 1, 2, 48, 160, 64, 64
    g = torch.Generator().manual_seed(17)
    scene = O.synthetic_scene(n, v, H, W, C, seed=17, intrinsics=O.K_KITTIRAW, smooth=True)
    net = build_net(O.FieldConfig(), O.init_mlp(C + 39, 64, 0, gen=g), scene, [0], device=DEV)
    wrapped = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=True)).bind_parallel(net).eval().to(DEV)
    sampler = bts.ImageRaySampler(3.0, 80.0)
    jitter = torch.rand(n * v * H * W, K, generator=g).to(DEV)
    inputs = [scene[k].to(DEV) for k in ("images", "projs", "poses")]
    kw = dict(ids_encoder=[0], ids_render=[0], jitter=jitter)
    x = 3 + 60 * torch.rand(4000, generator=g)
    pts = torch.stack([x, x * (torch.rand(4000, generator=g) - 0.5), x * 0.3 * (torch.rand(4000, generator=g) - 0.5), torch.rand(4000, generator=g)], dim=1).to(DEV)
    P32 = torch.tensor([[80.5, -150.0, 0.4, 1.0], [24.5, 0.3, -150.0, 2.0], [1.0, 0.002, 0.003, 0.27]], device=DEV)
    P64 = torch.tensor([[0.01, -1.9, 0.004, 0.01], [0.01, 0.003, -6.2, 0.02], [1.0, 0.002, 0.003, 0.27]], device=DEV, dtype=torch.float64)
    for P, convention, eigen in ((P32, "kitti_raw", True), (P64, "kitti_360", False)):
        gt = bts.load_depth(pts, P, (H, W), convention, eigen)
        assert int((gt != 0).sum()) > 200
        ev, ev_gt = (bts.FusedDepthEval(wrapped, sampler, depth_scaling="median", capacity=2) for _ in range(2))
        data = ev.frame_lidar(*inputs, pts, P, convention, eigen, **kw)
        want = ev_gt.frame(*inputs, gt.float(), **kw)
        assert ev.n_frames == 1 and torch.equal(ev.rows[0], ev_gt.rows[0]) and bool(torch.isfinite(ev.rows[0]).all())
        assert torch.equal(data["depth_metrics_row"], want["depth_metrics_row"]) and torch.equal(data["depth_gt"], gt.float())
        assert data["depth_gt"].shape == (1, H, W) and ev.rows[0, 9].item() == float((gt != 0).sum())
        nvs, nvs_gt = (bts.FusedNVSEval(wrapped, sampler, (H, W), capacity=2) for _ in range(2))
        d2 = nvs.frame_lidar(*inputs, pts, P, convention, eigen, **kw)
        w2 = nvs_gt.frame(*inputs, gt.float(), **kw)
        assert torch.equal(nvs.rows[0], nvs_gt.rows[0]) and torch.equal(nvs.depth.rows[0], nvs_gt.depth.rows[0])
        assert torch.equal(d2["depth_metrics_row"], w2["depth_metrics_row"])
    torch.cuda.synchronize()
