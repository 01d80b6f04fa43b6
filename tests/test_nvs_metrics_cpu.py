"""NVS evaluation metrics, the part that needs no GPU: the restatement the GPU tests lean on (tests/_nvs_metrics_oracle.py:
scipy.ndimage.uniform_filter on float64 arrays under skimage's formulas) against the golden fixture (tests/golden/nvs_metrics.npz), the
crop bounds, the resize index against F.interpolate, the ABI additions and the host-only error paths of bts_nvs_metrics.

The restatement is held to the stored rows within 1e-13 (ssim, ssim_c*) and 1e-14 relative (mse), not to the bit: numpy's pairwise
sums may pick another vector width on another CPU.  Those are the distances the generator allows between its two summation orders."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import behindthescenes_amd as bts
from behindthescenes_amd import _lib, native
from behindthescenes_amd.build import build_library

from tests import _nvs_metrics_oracle as NO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nvs_metrics.npz")
EVAL = dict(a=(31, 50), b=(20, 33), c=(9, 9), d=(30, 58))
CROP = dict(a=(27, 44), b=(18, 29), c=(7, 7), d=(26, 52), g=(172, 576))


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def close_rows(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = np.all(np.abs(got[..., [0, 3, 4, 5]] - want[..., [0, 3, 4, 5]]) <= 1e-13) and np.all(np.abs(got[..., 2] - want[..., 2]) <= 1e-14 * want[..., 2])
    psnr = np.where(np.isinf(want[..., 1]), got[..., 1] == want[..., 1], np.abs(got[..., 1] - np.where(np.isinf(want[..., 1]), 0, want[..., 1])) <= 1e-12)
    return bool(ok and np.all(psnr) and np.array_equal(got[..., 6:], want[..., 6:]))


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_restatement_reproduces_the_golden_rows(gold, name):
    row = NO.evaluate(gold[f"{name}_pred"], gold[f"{name}_gt"], EVAL[name])
    assert close_rows(row, gold[f"{name}_row"]), (row, gold[f"{name}_row"])
    assert (row[6], row[7]) == ((CROP[name][0] - 6) * (CROP[name][1] - 6), CROP[name][0] * CROP[name][1])
    assert close_rows(NO.evaluate_direct(gold[f"{name}_pred"], gold[f"{name}_gt"], EVAL[name]), gold[f"{name}_row"])


def test_restatement_on_equal_images_the_frames_and_the_real_size(gold):
    e = NO.evaluate(gold["a_gt"], gold["a_gt"], EVAL["a"])
    assert close_rows(e, gold["e_row"]) and e[2] == 0 and e[1] == math.inf and abs(e[0] - 1) <= 1e-13
    preds, gts = np.concatenate((gold["a_pred"][None], gold["m_pred"])), np.concatenate((gold["a_gt"][None], gold["m_gt"]))
    assert np.array_equal(gold["m_rows"][0], gold["a_row"])
    for i in range(3):
        assert close_rows(NO.evaluate(preds[i], gts[i], EVAL["a"]), gold["m_rows"][i]), i
    assert len({r[0] for r in gold["m_rows"]}) == 3
    pred, gt = NO.inputs_g()
    g = NO.evaluate(pred, gt, (192, 640))
    assert close_rows(g, gold["g_row"]), (g, gold["g_row"])
    assert (g[6], g[7]) == (166 * 570, 172 * 576)


def test_fixture_is_what_the_generator_writes(gold):
    sys.path.insert(0, os.path.dirname(GOLDEN))
    try:
        import gen_golden_nvs_metrics as gen
        fresh = gen.generate()          # asserts the two summation orders and every mutant on the way
    finally:
        sys.path.pop(0)
    assert sorted(fresh) == sorted(gold)
    for k in gold:
        a, b = np.asarray(fresh[k]), gold[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if k == "meta":
            continue
        if k.endswith("_row") or k.endswith("_rows"):
            assert close_rows(a, b), k
        else:
            assert np.array_equal(a, b), k


@pytest.mark.parametrize("size", [(9, 9), (20, 33), (31, 50), (30, 58), (100, 20), (140, 60), (192, 640), (256, 384), (375, 1242)])
def test_crop_bounds_are_the_references_expressions(size):
    h, w = size
    want = (int(math.ceil(0.05 * h)), int(math.floor(0.95 * h)), int(math.ceil(0.05 * w)), int(math.floor(0.95 * w)))      # evaluator_nvs.py:158-161
    assert native.nvs_crop_box(size) == want == NO.crop_box(h, w)
    literal = {(100, 20): (5, 95, 1, 19), (20, 33): (1, 19, 2, 31), (192, 640): (10, 182, 32, 608), (9, 9): (1, 8, 1, 8), (31, 50): (2, 29, 3, 47)}
    if size in literal:
        assert want == literal[size]
    if size in ((31, 50), (20, 33), (9, 9), (30, 58), (192, 640)):
        name = {(31, 50): "a", (20, 33): "b", (9, 9): "c", (30, 58): "d", (192, 640): "g"}[size]
        assert (want[1] - want[0], want[3] - want[2]) == CROP[name]


@pytest.mark.parametrize("sizes", [((24, 40), (31, 50)), ((48, 70), (20, 33)), ((26, 30), (44, 58))])
def test_resize_index_formula_is_f_interpolate(sizes):
    (H, W), (He, We) = sizes
    src = torch.arange(H * W * 3, dtype=torch.float32).view(H, W, 3)
    want = F.interpolate(src.permute(2, 0, 1)[None], (He, We))[0].permute(1, 2, 0)
    assert np.array_equal(NO.resize_nearest(src.numpy(), He, We), want.numpy())


def test_symbols_and_abi_version(lib):
    for name in ("bts_nvs_metrics", "bts_nvs_metrics_workspace"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.bts_abi_version() == _lib.ABI_VERSION == 9
    assert bts.FusedNVSEval is bts.nvs_metrics.FusedNVSEval and bts.compute_nvs_metrics is bts.nvs_metrics.compute_nvs_metrics
    assert {"FusedNVSEval", "compute_nvs_metrics", "nvs_metrics"} <= set(bts.__all__)
    assert bts.nvs_metrics.METRIC_KEYS == ("ssim", "psnr") and bts.nvs_metrics.ROW_KEYS == NO.ROW_KEYS


def test_the_new_struct_matches_the_c_layout():
    fields = [f[0] for f in _lib.BtsNvsMetrics._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bts_render.h"\nint main(void) {\n  printf("%zu", sizeof(BtsNvsMetrics));\n' + \
        "".join(f'  printf(" %zu", offsetof(BtsNvsMetrics, {f}));\n' for f in fields) + \
        '  printf(" %d %d", BTS_NVS_METRICS_MAX_FRAMES, BTS_NVS_METRICS_ROW);\n  return 0;\n}\n'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(root, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(_lib.BtsNvsMetrics)] + [getattr(_lib.BtsNvsMetrics, f).offset for f in fields] + \
        [_lib.BTS_NVS_METRICS_MAX_FRAMES, _lib.BTS_NVS_METRICS_ROW]
    assert (_lib.BtsNvsMetrics.gt.offset, _lib.BtsNvsMetrics.B.offset, _lib.BtsNvsMetrics.data_range.offset) == (40, 80, 120)


def test_host_only_error_paths(lib):
    assert lib.bts_nvs_metrics(None, None, 0, None) == -1 and b"NULL" in lib.bts_last_error()

    def args(**kw):
        a = _lib.BtsNvsMetrics(pred=16, pred_sb=24 * 40 * 3, pred_sy=120, pred_sx=3, pred_sc=1, gt=16, gt_sb=24 * 40 * 3, gt_sy=120, gt_sx=3, gt_sc=1,
                               B=1, H=24, W=40, He=31, We=50, y0=2, y1=29, x0=3, x1=47, data_range=1.0, metrics=16)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    need = lib.bts_nvs_metrics_workspace(1, 31, 50)
    assert need > 0
    call = lambda a, ws=16, n=None: lib.bts_nvs_metrics(C.byref(a), ws, need if n is None else n, None)
    for bad in (dict(pred=None), dict(gt=None), dict(metrics=None), dict(H=0), dict(W=-1), dict(He=0), dict(We=0), dict(B=0), dict(B=-2)):
        assert call(args(**bad)) == -1 and b"NULL pointer or non-positive size" in lib.bts_last_error(), bad
    assert call(args(B=65), n=1 << 30) == -1 and b"B=65" in lib.bts_last_error()
    for bad in (dict(y0=-1), dict(x0=-1), dict(y1=32), dict(x1=51), dict(y0=30, y1=29), dict(x0=48, x1=47)):
        assert call(args(**bad)) == -1 and b"crop box" in lib.bts_last_error(), bad
    for bad in (dict(y1=8), dict(x1=9), dict(y0=23), dict(x0=41)):          # a side of 6
        assert call(args(**bad)) == -1 and b"7-pixel window" in lib.bts_last_error(), bad
    for bad in (0.0, -1.0, math.nan):
        assert call(args(data_range=bad)) == -1 and b"data_range" in lib.bts_last_error(), bad
    assert call(args(H=1 << 16, W=1 << 15)) == -1 and b"2^30" in lib.bts_last_error()
    assert call(args(He=1 << 16, We=1 << 15, y1=29, x1=47), n=1 << 40) == -1 and b"2^30" in lib.bts_last_error()
    assert call(args(), n=need - 1) == -1 and b"workspace" in lib.bts_last_error()
    assert call(args(), ws=None) == -1 and b"workspace" in lib.bts_last_error()
    assert call(args(), ws=24) == -1 and b"aligned" in lib.bts_last_error()


def test_workspace_size(lib):
    ws = lib.bts_nvs_metrics_workspace
    one = ws(1, 192, 640)
    assert one >= 11 * 18 * 4 * 8 and one % 16 == 0          # the 172 x 576 crop: 166 x 570 interior pixels in 16 x 32 tiles
    assert ws(2, 192, 640) > one and ws(64, 192, 640) > ws(63, 192, 640)
    assert ws(1, 9, 9) > 0 and ws(1, 3, 3) > 0
    for bad in ((0, 31, 50), (-1, 31, 50), (65, 31, 50), (1, 0, 50), (1, 31, -3), (1, 1 << 16, 1 << 15)):
        assert ws(*bad) == 0, bad


def test_cpu_tensors_and_bad_arguments_are_refused(gold):
    pred, gt = torch.from_numpy(gold["a_pred"])[None, None, :, :, None], torch.from_numpy(gold["a_gt"])[None, None]
    with pytest.raises(bts.BtsNativeError, match="must live on the GPU"):
        bts.compute_nvs_metrics(pred, gt, (31, 50))
    with pytest.raises(bts.BtsNativeError, match="must live on the GPU"):
        native.nvs_metrics(pred[:, 0, :, :, 0], gt[:, 0], (31, 50))
    with pytest.raises(bts.BtsNativeError, match=r"rgb_gt: \(1, v, H, W, 3\) expected"):
        bts.compute_nvs_metrics(pred, gt[0], (31, 50))
    with pytest.raises(bts.BtsNativeError, match="rgb_pred"):
        bts.compute_nvs_metrics(pred[..., 0, :], gt, (31, 50))
    with pytest.raises(bts.BtsNativeError, match="eval_resolution"):
        bts.compute_nvs_metrics(pred, gt, 31)
    with pytest.raises(bts.BtsNativeError, match="eval_resolution"):
        bts.FusedNVSEval(None, None, (0, 50))
    with pytest.raises(bts.BtsNativeError, match="capacity"):
        bts.FusedNVSEval(None, None, (31, 50), capacity=0)
    ev = bts.FusedNVSEval(None, None, (31, 50), capacity=2)
    with pytest.raises(bts.BtsNativeError, match="must live on the GPU"):
        ev.update(pred, gt)
    with pytest.raises(bts.BtsNativeError, match="no frame"):
        ev.compute()
    with pytest.raises(bts.BtsNativeError, match="is not the frame size"):
        ev.frame(torch.zeros(1, 3, 3, 24, 40), None, None)
    assert ev.n_frames == 0
