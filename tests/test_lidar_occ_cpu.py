"""LiDAR occupancy evaluation, the part that needs no GPU: the torch restatement the GPU tests and the probe lean on
(tests/_lidar_occ_oracle.py) against the golden fixture from the real reference (tests/golden/lidar_occ.npz), the host side of the
package (get_pts, the metrics from the six counts) and the host-only error paths of the three entry points."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import _lib, native
from behindthescenes_amd import lidar_occupancy as L
from behindthescenes_amd.build import build_library

from tests import _lidar_occ_oracle as LO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar_occ.npz")
X_RANGE, Z_RANGE = (-4, 4), (20, 4)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def case_of(gold, name):
    g = {k[len(name) + 1:]: gold[k] for k in gold.files if k.startswith(name + "_")}
    t = {k: torch.from_numpy(v) for k, v in g.items() if v.ndim > 0 and k not in ("offsets", "counts", "metrics")}
    off = g["offsets"].tolist()
    t["clouds"] = [t["points"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    t["y_res"], t["offsets"], t["counts"], t["metrics"] = int(g["y_res"]), off, g["counts"].tolist(), g["metrics"]
    return t


def same_values(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_reproduces_the_reference_bit_for_bit(gold, name):
    c = case_of(gold, name)
    y_range, max_dist, min_dist = tuple(gold["y_range"].tolist()), float(gold["max_dist"]), int(gold["min_dist"])
    tables = LO.lidar_tables(c["clouds"], c["velo_poses"], y_range, c["y_res"], max_dist)
    assert tables.shape == c["tables"].shape == (c["y_res"], len(c["clouds"]), 362, 2)
    assert torch.equal(tables, c["tables"])
    # the fixture really has leading and interior empty bins (carried values) in every table
    raw = c["tables"][:, :, 1:-1, 1]
    assert bool((raw[:, :, 1:] == raw[:, :, :-1]).any(dim=-1).all())
    occ, vis = LO.check_occupancy(c["q_pts"], c["tables"], c["velo_poses"], min_dist)
    assert torch.equal(occ, c["is_occupied"]) and torch.equal(vis, c["is_visible"])
    dist, pred, _ = LO.predicted_visibility(c["q_pts"], torch.from_numpy(gold["proj"]), c["cam_pose"], torch.from_numpy(gold["depth"]))
    assert torch.equal(dist <= pred, c["is_visible_pred"])
    values, (Pm, Om, Vm) = LO.metrics(occ, vis, dist <= pred, c["sigma"] > float(gold["occ_threshold"]))
    assert torch.equal(Pm, c["mask_P"]) and torch.equal(Om, c["mask_O"]) and torch.equal(Vm, c["mask_V"])
    assert same_values([values[k] for k in L.METRIC_KEYS], c["metrics"])
    assert LO.cell_counts(Pm, Om, Vm) == c["counts"]
    if name == "b":     # remainder points: untouched by every slice
        rest = c["q_pts"].shape[0] % c["y_res"]
        assert rest == 2 and not c["is_visible"][-rest:].any() and not c["is_occupied"][-rest:].any()
    assert int((~c["decided"]).sum()) <= c["q_pts"].shape[0] // 100


def test_host_side_of_the_package_matches_the_reference(gold):
    a, b = case_of(gold, "a"), case_of(gold, "b")
    y_range = tuple(gold["y_range"].tolist())
    pts, dims = L.get_pts(X_RANGE, y_range, Z_RANGE, 10, 4, 1)
    assert dims == (80, 1, 160) and tuple(pts.shape) == (1, 160, 80, 3) and torch.equal(pts.reshape(-1, 3), a["q_pts"])
    pts, dims = L.get_pts(X_RANGE, y_range, Z_RANGE, 5, 4, 3)
    assert dims == (40, 3, 80) and torch.equal(pts.reshape(-1, 3)[:-1], b["q_pts"])
    assert L.get_pts(X_RANGE, y_range, Z_RANGE, 10, 4)[1] == (80, 3, 160)          # y_res from ppm_y
    for c in (a, b):
        m = L.metrics_from_counts(c["counts"])
        assert tuple(m) == L.METRIC_KEYS
        assert same_values([float(m[k]) for k in L.METRIC_KEYS], c["metrics"])
        for k in ("o_acc", "o_rec", "o_prec", "ie_acc", "ie_r", "t_ie"):
            assert isinstance(m[k], float)
        for k in ("ie_rec", "ie_prec", "t_no_nop_nv"):
            assert isinstance(m[k], torch.Tensor) and m[k].dim() == 0
    assert math.isnan(float(L.metrics_from_counts([3, 4, 0, 0, 0, 0])["ie_acc"]))     # a mean over an empty selection
    assert bts.FusedOccupancyEval is L.FusedOccupancyEval


def test_host_only_error_paths(lib):
    off = (C.c_int32 * 34)(*[400 * i for i in range(34)])
    ok = lambda T=4, y_res=1, o=off, pts=16: lib.bts_lidar_slices(pts, o, T, 16, 16, 0.0, 0.75, y_res, 20.0, 16, 16, None)
    assert lib.bts_lidar_slices(None, off, 4, 16, 16, 0.0, 0.75, 1, 20.0, 16, 16, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_lidar_slices(16, None, 4, 16, 16, 0.0, 0.75, 1, 20.0, 16, 16, None) == -1
    assert ok(T=33) == -2 and b"32 clouds" in lib.bts_last_error()
    assert ok(y_res=17) == -2 and b"16 slices" in lib.bts_last_error()
    assert ok(T=0) == -1 and ok(y_res=0) == -1
    assert ok(pts=20) == -1 and b"aligned" in lib.bts_last_error()
    bad = (C.c_int32 * 5)(0, 400, 1200, 800, 1600)
    assert ok(o=bad) == -1 and b"monotone" in lib.bts_last_error()
    assert ok(o=(C.c_int32 * 5)(8, 400, 800, 1200, 1600)) == -1 and b"offsets[0]" in lib.bts_last_error()
    small = (C.c_int32 * 5)(0, 400, 759, 1200, 1600)
    assert ok(o=small) == -2 and b"cloud 1 has 359 points" in lib.bts_last_error()
    assert lib.bts_lidar_slices_workspace(4, 1) >= 4 * 360 * 4 + 4 * 8 and lib.bts_lidar_slices_workspace(33, 1) == 0

    assert lib.bts_lidar_occupancy(None, 10, 16, 1, 4, 16, 3.0, 16, 16, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_lidar_occupancy(16, 0, 16, 1, 4, 16, 3.0, 16, 16, None) == -1
    assert lib.bts_lidar_occupancy(16, 10, 16, 1, 33, 16, 3.0, 16, 16, None) == -2 and b"32 clouds" in lib.bts_last_error()
    assert lib.bts_lidar_occupancy(16, 10, 16, 17, 4, 16, 3.0, 16, 16, None) == -2

    cfg = native._spec_cfg(native.FieldSpec(C=64, d_hidden=64, n_blocks=0), n=1, H=48, W=160)
    tens = _lib.BtsFieldTensors(*([16] * 9))
    assert lib.bts_occupancy_eval(None, None, None, None, 0, None) == -1 and b"NULL" in lib.bts_last_error()
    assert lib.bts_occupancy_eval(C.byref(cfg), C.byref(tens), None, None, 0, None) == -1 and b"NULL" in lib.bts_last_error()

    def args(**kw):
        a = _lib.BtsOccupancyEval(q_pts=16, P=100, T=4, y_res=1, H=48, W=160, points=16, offsets=C.cast(off, C.c_void_p).value, velo_poses=16,
                                  borders361=16, y_lo=0.0, y_hi=0.75, max_dist=20.0, min_dist=3.0, occ_threshold=0.5, pred_depth_z=16, proj=16,
                                  cam_pose=16, counts=16)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    ev = lambda a, c=cfg, ws=None, n=0: lib.bts_occupancy_eval(C.byref(c), C.byref(tens), C.byref(a), ws, n, None)
    assert ev(args(counts=None)) == -1 and ev(args(P=0)) == -1
    assert ev(args(T=33)) == -2 and ev(args(y_res=17)) == -2
    assert ev(args(offsets=C.cast(bad, C.c_void_p).value)) == -1 and b"monotone" in lib.bts_last_error()
    assert ev(args(offsets=C.cast(small, C.c_void_p).value)) == -2
    two = native._spec_cfg(native.FieldSpec(C=64, d_hidden=64, n_blocks=0), n=2, H=48, W=160)
    assert ev(args(), c=two) == -1 and b"n = 1" in lib.bts_last_error()
    unsupported = native._spec_cfg(native.FieldSpec(C=48, d_hidden=64, n_blocks=0), n=1, H=48, W=160)
    assert ev(args(), c=unsupported) == -2 and b"envelope" in lib.bts_last_error()
    need = lib.bts_occupancy_eval_workspace(100, 4, 1)
    assert need >= 4 * 360 * 4 + 4 * 362 * 8 + 5 * 64 + 2 * 100 + 400 and lib.bts_occupancy_eval_workspace(100, 33, 1) == 0
    assert ev(args()) == -4 and ev(args(), ws=16, n=need - 1) == -4 and b"workspace" in lib.bts_last_error()


def test_the_new_struct_matches_the_c_layout():
    fields = [f[0] for f in _lib.BtsOccupancyEval._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bts_render.h"\nint main(void) {\n  printf("%zu", sizeof(BtsOccupancyEval));\n' + \
        "".join(f'  printf(" %zu", offsetof(BtsOccupancyEval, {f}));\n' for f in fields) + "  return 0;\n}\n"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(root, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(_lib.BtsOccupancyEval)] + [getattr(_lib.BtsOccupancyEval, f).offset for f in fields]


def test_cpu_tensors_and_torch_mode_nets_are_refused(gold):
    a = case_of(gold, "a")
    with pytest.raises(bts.BtsNativeError, match="must live on the GPU"):
        L.get_lidar_slices(a["clouds"], a["velo_poses"], (0, .75), 1, 20.4)
    slices = [[a["tables"][0, j] for j in range(4)]]
    with pytest.raises(bts.BtsNativeError):
        L.check_occupancy(a["q_pts"], slices, a["velo_poses"])
    conf = dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=False, code_mode="z", sample_color=False,
                code=dict(num_freqs=6, freq_factor=1.5, include_input=True), encoder=dict(type="feature_map", size=(8, 16), d_out=64),
                mlp_coarse=dict(type="resnet", n_blocks=0, d_hidden=64), mlp_fine=dict(type="empty"))
    net = bts.BTSNet(conf)
    assert net.torch_mode
    with pytest.raises(bts.BtsNativeError, match="PyTorch composition"):
        L.FusedOccupancyEval(net)(a["clouds"], a["velo_poses"], torch.zeros(48, 160), torch.eye(3), torch.eye(4))


@pytest.mark.needs_reference
def test_fixture_is_what_the_reference_generates(gold):
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN)))
    try:
        import gen_golden_lidar_occ as gen
        fresh = gen.generate()
    finally:
        sys.path.pop(0)
    assert sorted(fresh) == sorted(gold.files)
    for k in gold.files:
        a, b = np.asarray(fresh[k]), gold[k]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
