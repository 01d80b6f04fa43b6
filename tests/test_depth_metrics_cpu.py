"""Depth evaluation metrics, the part that needs no GPU: the torch restatement the GPU tests and the probe lean on
(tests/_depth_metrics_oracle.py) against the golden fixture from the real reference (tests/golden/depth_metrics.npz), the resize index
formula against F.interpolate, and the host-only error paths of bts_depth_metrics.

Case c (l2): LAPACK's fp32 least squares is not reproducible to the bit on the CPU (its result moves with the alignment of its
operands, run to run), so the restatement is pinned with the coefficients the reference's own call returned (the fixture's c_scale32);
its own lstsq call is held to those within 1e-5 relative -- a hundred times the distance the fixture records between the fp32 and fp64
solutions of this system."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import behindthescenes_amd as bts
from behindthescenes_amd import _lib
from behindthescenes_amd.build import build_library

from tests import _depth_metrics_oracle as DO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_metrics.npz")
MODES = dict(a="median", b="median", c="l2", d=None, e="median")
UNREPRODUCIBLE = ("c_metrics32", "c_metrics64", "c_scale32", "c_counts", "meta")      # downstream of LAPACK's fp32 lstsq


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def inputs_of(gold, name):
    pred = gold["b_pred"] if name == "b" else gold["a_pred"]
    gt = gold["b_gt"] if name == "b" else gold["e_gt"] if name == "e" else gold["a_gt"]
    return torch.from_numpy(pred)[None, None], torch.from_numpy(gt)[None, None]


def same_values(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool(a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True))


def check_case(gold, name, pred, gt, mode):
    coeffs = gold[f"{name}_scale32"].tolist() if mode == "l2" else None
    r = DO.evaluate(pred, gt, mode, coeffs=coeffs)
    got = np.array([r["metrics"][k].item() for k in DO.METRIC_KEYS], dtype=np.float32)
    assert all(r["metrics"][k].dtype == torch.float32 and r["metrics"][k].dim() == 0 for k in DO.METRIC_KEYS)
    assert same_values(got, gold[f"{name}_metrics32"]), (name, got, gold[f"{name}_metrics32"])
    assert r["counts"] == gold[f"{name}_counts"].tolist()
    assert same_values(np.array([r["scale"].item(), r["shift"].item()], dtype=np.float32), gold[f"{name}_scale32"])
    return r


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_restatement_reproduces_the_reference_bit_for_bit(gold, name):
    pred, gt = inputs_of(gold, name)
    r = check_case(gold, name, pred, gt, MODES[name])
    n_metric, n_scale = r["counts"][:2]
    if name == "a":
        assert n_scale % 2 == 1 and 0.3 < n_scale / gt.numel() < 0.5 and torch.unique(gt[gt > 0]).numel() < n_scale
    if name == "b":
        assert n_scale % 2 == 0 and n_scale == gt.numel() - 1
        assert gold["b_medians"][0] == torch.sort(gt[gt > 0])[0][n_scale // 2 - 1].item() < torch.sort(gt[gt > 0])[0][n_scale // 2].item()
    if name == "c":
        own = DO.evaluate(pred, gt, "l2")
        x = np.array([own["scale"].item(), own["shift"].item()], dtype=np.float64)
        assert np.all(np.abs(x - gold["c_scale32"]) <= 1e-5 * np.abs(gold["c_scale32"]))
        assert np.all(np.abs(gold["c_scale32"] - gold["c_x64"]) <= 1e-6 * np.abs(gold["c_x64"]))
        assert json.loads(str(gold["meta"]))["c"]["fp32_lstsq_rel_distance_from_fp64"][0] < 1e-6
    if name == "d":
        assert gold["d_scale32"].tolist() == [1.0, 0.0]
    if name == "e":
        assert n_metric == n_scale + 3 and np.isnan(gold["e_metrics32"][3]) and gold["e_scale32"][0] == gold["a_scale32"][0]


def test_restatement_on_the_three_frames_of_case_f(gold):
    for i in range(3):
        pred, gt = torch.from_numpy(gold["f_pred"][i])[None, None], torch.from_numpy(gold["f_gt"][i])[None, None]
        r = DO.evaluate(pred, gt, "median")
        assert same_values(np.array([r["metrics"][k].item() for k in DO.METRIC_KEYS], dtype=np.float32), gold["f_metrics32"][i])
        assert r["counts"] == gold["f_counts"][i].tolist() and np.float32(r["scale"].item()) == gold["f_scale32"][i][0]


@pytest.mark.parametrize("sizes", [((26, 30), (44, 58)), ((24, 80), (47, 155)), ((192, 640), (375, 1242))])
def test_resize_index_formula_is_f_interpolate(sizes):
    (H, W), (Hg, Wg) = sizes
    src = torch.arange(H * W, dtype=torch.float32).view(1, 1, H, W)
    assert torch.equal(DO.resize_nearest(src, Hg, Wg), F.interpolate(src, (Hg, Wg)))
    if (H, W) == (26, 30):      # the sizes at which the fp32 formula is not the exact rational
        assert (DO.nearest_index(Hg, H) != DO.exact_index(Hg, H)).any() and (DO.nearest_index(Wg, W) != DO.exact_index(Wg, W)).any()


def test_host_only_error_paths(lib):
    assert lib.bts_depth_metrics(None, None, 0, None) == -1 and b"NULL" in lib.bts_last_error()

    def args(**kw):
        a = _lib.BtsDepthMetrics(pred=16, H=26, W=30, gt=16, Hg=44, Wg=58, B=1, mode=1, clamp_lo=1e-3, clamp_hi=80.0, metrics=16, counts=None)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    need = lib.bts_depth_metrics_workspace(1, 44, 58, 1)
    call = lambda a, ws=16, n=None: lib.bts_depth_metrics(C.byref(a), ws, need if n is None else n, None)
    for bad in (dict(pred=None), dict(gt=None), dict(metrics=None), dict(H=0), dict(W=-1), dict(Hg=0), dict(Wg=0), dict(B=0)):
        assert call(args(**bad)) == -1 and b"NULL pointer or non-positive size" in lib.bts_last_error(), bad
    assert call(args(mode=3)) == -1 and b"unknown mode 3" in lib.bts_last_error()
    assert call(args(mode=-1)) == -1 and b"unknown mode" in lib.bts_last_error()
    assert call(args(B=65), n=1 << 30) == -1 and b"B=65" in lib.bts_last_error()
    assert call(args(Hg=1 << 16, Wg=1 << 15), n=1 << 40) == -1 and b"2^30" in lib.bts_last_error()
    assert call(args(), n=need - 1) == -1 and b"workspace" in lib.bts_last_error()
    assert call(args(), ws=None) == -1 and b"workspace" in lib.bts_last_error()
    assert call(args(), ws=24) == -1 and b"aligned" in lib.bts_last_error()


def test_workspace_size(lib):
    ws = lib.bts_depth_metrics_workspace
    one = ws(1, 375, 1242, 1)
    assert one >= 3 * 2 * 2048 * 4 + (375 * 1242 + 2047) // 2048 * 64 and one % 16 == 0
    assert ws(2, 375, 1242, 1) > one and ws(64, 375, 1242, 1) > ws(63, 375, 1242, 1) > ws(2, 375, 1242, 1)
    assert ws(1, 44, 58, 0) > 0 and ws(1, 44, 58, 2) > 0
    for bad in ((0, 44, 58, 1), (65, 44, 58, 1), (1, 0, 58, 1), (1, 44, -3, 1), (1, 44, 58, 3), (1, 44, 58, -1), (1, 1 << 16, 1 << 15, 1)):
        assert ws(*bad) == 0, bad


def test_the_new_struct_matches_the_c_layout():
    fields = [f[0] for f in _lib.BtsDepthMetrics._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bts_render.h"\nint main(void) {\n  printf("%zu", sizeof(BtsDepthMetrics));\n' + \
        "".join(f'  printf(" %zu", offsetof(BtsDepthMetrics, {f}));\n' for f in fields) + \
        '  printf(" %d %d", BTS_DEPTH_METRICS_MAX_FRAMES, BTS_DEPTH_METRICS_ROW);\n  return 0;\n}\n'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(root, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(_lib.BtsDepthMetrics)] + [getattr(_lib.BtsDepthMetrics, f).offset for f in fields] + \
        [_lib.BTS_DEPTH_METRICS_MAX_FRAMES, _lib.BTS_DEPTH_METRICS_ROW]


def test_cpu_tensors_are_refused(gold):
    pred, gt = inputs_of(gold, "a")
    with pytest.raises(bts.BtsNativeError, match="must live on the GPU"):
        bts.compute_depth_metrics(pred, gt, "median")
    with pytest.raises(bts.BtsNativeError, match="one frame expected"):
        bts.compute_depth_metrics(torch.zeros(2, 1, 4, 4), gt)
    with pytest.raises(bts.BtsNativeError, match="depth_scaling"):
        bts.FusedDepthEval(None, None, depth_scaling="mean")
    with pytest.raises(bts.BtsNativeError, match="capacity"):
        bts.FusedDepthEval(None, None, capacity=0)
    ev = bts.FusedDepthEval(None, None, depth_scaling="median", capacity=2)
    with pytest.raises(bts.BtsNativeError, match="must live on the GPU"):
        ev.update(pred, gt)
    with pytest.raises(bts.BtsNativeError, match="no frame"):
        ev.compute()
    assert bts.depth_metrics.METRIC_KEYS == DO.METRIC_KEYS and bts.FusedDepthEval is bts.depth_metrics.FusedDepthEval


@pytest.mark.needs_reference
def test_fixture_is_what_the_reference_generates(gold):
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN)))
    try:
        import gen_golden_depth_metrics as gen
        fresh = gen.generate()
    finally:
        sys.path.pop(0)
    assert sorted(fresh) == sorted(gold)
    for k in gold:
        a, b = np.asarray(fresh[k]), gold[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if k in UNREPRODUCIBLE:      # (the generator has asserted them against the restatement with the coefficients of ITS run)
            continue
        if k == "c_x64":
            assert np.allclose(a, b, rtol=1e-12, atol=0), k
            continue
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
    # the live run's fp32 least squares lands within 1e-5 relative of the stored one
    assert np.all(np.abs(fresh["c_scale32"].astype(np.float64) - gold["c_scale32"]) <= 1e-5 * np.abs(gold["c_scale32"]))
