"""CPU (no GPU): the numpy oracle of the LiDAR ground-truth depth map (tests/_lidar_depth_oracle.py) against the golden of the REAL
reference (tests/golden/lidar_depth.npz, written by tests/golden/gen_golden_lidar_depth.py from the reference's two ``load_depth``
functions), the closed form against a literal statement of the eight rules on random clouds, and the Python argument checks that need
no library."""
import os

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import lidar_depth, native
from tests import _lidar_depth_oracle as LD

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar_depth.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def case_of(gold, name):
    convention = "kitti_raw" if name.startswith("kitti_raw") else "kitti_360"
    return dict(points=gold[name + "_points"], P=gold[name + "_P"], depth=gold[name + "_depth"], src=gold[name + "_src"],
                size=tuple(gold[name + "_depth"].shape[1:]), convention=convention, eigen=name.endswith("_eigen"))


def test_the_golden_holds_every_case_the_fixture_is_meant_to(gold):
    names = set(gold["names"].tolist())
    want = {f"{c}_{h}x{w}_{t}" for c in LD.CONVENTIONS for h, w in ((1, 2), (2, 2), (5, 7), (24, 40)) for t in ("f32", "f64")}
    want |= {f"kitti_raw_{s}_{t}_eigen" for s in ("5x7", "24x40") for t in ("f32", "f64")}
    assert names == want
    for name in names:
        c = case_of(gold, name)
        assert c["P"].dtype == (np.float32 if "_f32" in name else np.float64) and c["points"].dtype == np.float32
        assert c["depth"].dtype == np.float64 and c["depth"].shape == (1,) + c["size"]      # the reference holds float64


def test_oracle_equals_the_reference_on_every_golden_case(gold):
    """the occupied pixels are equal and the values are the reference's, bit for bit, in the reference's dtype (P's, held as float64)"""
    for name in gold["names"].tolist():
        c = case_of(gold, name)
        mine, src = LD.load_depth(c["points"], c["P"], c["size"], c["convention"], c["eigen"], want_src=True)
        assert mine.dtype == c["P"].dtype and mine.shape == c["depth"].shape, name
        assert np.array_equal(mine != 0, c["depth"] != 0), name
        assert np.array_equal(mine.astype(np.float64), c["depth"]), name
        assert np.array_equal(src, c["src"]), name
        assert np.array_equal(LD.literal(c["points"], c["P"], c["size"], c["convention"], c["eigen"]).astype(np.float64), c["depth"]), name


def test_the_plain_z_buffer_is_a_different_function(gold):
    for name in gold["names"].tolist():
        c = case_of(gold, name)
        if c["size"][0] >= 2 and not (c["eigen"] and c["size"] == (24, 40)):
            z = LD.load_depth(c["points"], c["P"], c["size"], c["convention"], c["eigen"], mutant="zbuffer")
            assert not np.array_equal(z.astype(np.float64), c["depth"]), name


@pytest.mark.parametrize("convention", LD.CONVENTIONS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_closed_form_equals_the_eight_rules_on_random_clouds(convention, dtype):
    """300 clouds of 0 .. 60 points at 5 x 7: crowded pixels, many key pairs, points on both sides of the camera and outside the frame"""
    rng = np.random.default_rng(5 if convention == "kitti_raw" else 6)
    size, occupied = (5, 7), 0
    for trial in range(300):
        n = int(rng.integers(0, 61))
        if convention == "kitti_raw":
            P = np.array([[6.5, -6.0, 0.1, 1.25], [2.9, 0.2, -6.8, 1.5], [1.0, 0.03, 0.02, 0.5]])
        else:
            P = np.array([[0.02, -1.1, 0.01, -0.3], [-0.02, 0.03, -1.6, 0.1], [1.0, 0.03, 0.02, 0.5]])
        P = (P * (1 + 0.01 * rng.standard_normal((3, 4)))).astype(dtype)
        x = rng.uniform(-4, 12, n)
        pts = np.stack([x, x * rng.uniform(-0.6, 0.6, n), x * rng.uniform(-0.5, 0.5, n), rng.uniform(0, 1, n)], axis=1).astype(np.float32)
        for eigen in ((False, True) if convention == "kitti_raw" else (False,)):
            a = LD.load_depth(pts, P, size, convention, eigen)
            b = LD.literal(pts, P, size, convention, eigen)
            assert a.dtype == b.dtype == dtype and np.array_equal(a, b), (trial, eigen)
            occupied += int((a != 0).sum())
    assert occupied > 300


def test_python_argument_checks_need_no_library():
    pts, P = torch.zeros(3, 4), torch.zeros(3, 4)
    with pytest.raises(ValueError, match="convention"):
        lidar_depth.load_depth(pts, P, (5, 7), "kitti")
    with pytest.raises(ValueError, match="eigen_depth"):
        lidar_depth.load_depth(pts, P, (5, 7), "kitti_360", eigen_depth=True)
    with pytest.raises(ValueError, match="size"):
        lidar_depth.load_depth(pts, P, 5, "kitti_raw")
    with pytest.raises(bts.BtsNativeError, match="P:"):            # CPU tensors: no CPU path
        lidar_depth.load_depth(pts, P, (5, 7), "kitti_raw")
    with pytest.raises(bts.BtsNativeError, match="P:"):
        lidar_depth.load_depth(pts, P.half(), (5, 7), "kitti_raw")
    with pytest.raises(bts.BtsNativeError, match="P:"):
        lidar_depth.load_depth(pts, None, (5, 7), "kitti_raw")
    with pytest.raises(bts.BtsNativeError, match="P:"):
        lidar_depth.load_depth_batch(pts, (0, 3), P, (5, 7), "kitti_360")
    assert bts.load_depth is lidar_depth.load_depth and bts.load_depth_batch is lidar_depth.load_depth_batch
    assert callable(native.lidar_depth) and callable(bts.FusedDepthEval.frame_lidar) and callable(bts.FusedNVSEval.frame_lidar)


def test_library_rejects_what_the_reference_cannot_state_exactly():
    """host-only: the size query answers 0 for W < 2 and H * W >= 2^24, the entry BTS_E_UNSUPPORTED with a message, before any launch"""
    import ctypes as C
    from behindthescenes_amd import _lib
    from behindthescenes_amd.build import build_library
    build_library()
    lib = _lib.load()
    assert lib.bts_lidar_depth_workspace(1, 5, 1, 0) == 0 and lib.bts_lidar_depth_workspace(1, 4096, 4096, 0) == 0
    assert lib.bts_lidar_depth_workspace(33, 5, 7, 0) == 0 and lib.bts_lidar_depth_workspace(0, 5, 7, 0) == 0
    # four planes, each rounded up to 256 bytes, + the 256 the pointer's own rounding may cost; the fp64 key plane is twice as wide
    assert lib.bts_lidar_depth_workspace(1, 5, 7, 0) == 5 * 256 and lib.bts_lidar_depth_workspace(2, 24, 40, 1) == 256 + 3 * 7680 + 15360
    offs = (C.c_int64 * 2)(0, 0)

    def call(**kw):
        a = _lib.BtsLidarDepth(points=None, offsets=offs, P=16, B=1, H=5, W=7, convention=0, depth=16)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.bts_lidar_depth(C.byref(a), 16, 1 << 30, None), lib.bts_last_error()
    rc, msg = call(W=1)
    assert rc == -2 and b"W=1" in msg
    rc, msg = call(H=4096, W=4096)
    assert rc == -2 and b"2^24" in msg
    big = (C.c_int64 * 2)(0, 1 << 31)
    rc, msg = call(offsets=big, points=16)
    assert rc == -2 and b"2^31" in msg
    rc, msg = call(convention=2)
    assert rc == -1 and b"convention" in msg
    rc, msg = call(convention=1, eigen_depth=1)
    assert rc == -1 and b"eigen_depth" in msg
    rc, msg = call(B=33)
    assert rc == -1 and b"B=33" in msg
    assert lib.bts_lidar_depth(None, None, 0, None) == -1
    a = _lib.BtsLidarDepth(points=None, offsets=offs, P=16, B=1, H=5, W=7, convention=0, depth=16)
    assert lib.bts_lidar_depth(C.byref(a), None, 0, None) == -1 and b"workspace" in lib.bts_last_error()
