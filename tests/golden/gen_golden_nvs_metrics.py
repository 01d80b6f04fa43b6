"""Writes tests/golden/nvs_metrics.npz: the inputs of the small cases of tests/test_gpu_nvs_metrics.py and the expected rows of all of
them, from tests/_nvs_metrics_oracle.py (scipy.ndimage.uniform_filter on float64 arrays under skimage's formulas; skimage and lpips are
neither installed here nor part of the reference tree).

    python tests/golden/gen_golden_nvs_metrics.py

Cases (source -> eval_resolution, crop): a 24 x 40 -> 31 x 50 (27 x 44), b 48 x 70 -> 20 x 33 (18 x 29), c 9 x 9 (7 x 7, one window),
d 30 x 58 (26 x 52, flat 0.5 +- 1e-3), e pred == gt at a's sizes, m three frames at a's sizes (frame 0 is case a), g 192 x 640
(172 x 576; only its row is stored, _nvs_metrics_oracle.inputs_g regenerates the images).

What keeps the GPU tests' bars (1e-11 on ssim, 1e-12 relative on mse) honest is asserted here on every case:
  * a second evaluation that sums every window directly, in another order, stays within 1e-13 of the first for ssim / ssim_c* and
    within 1e-14 relative for mse;
  * the algorithmic mutants -- cov_norm = 1, a 2-pixel instead of a 3-pixel interior margin, a crop box one column short -- each move
    ssim by more than 1e-6 on the cases marked for them (MUTANT_CASES), five orders above the bar;
  * fp32 instead of fp64 arithmetic (what skimage >= 0.19 does with float32 images) moves ssim by more than the 1e-11 bar on its cases
    (about 1e-10 on noise; far more on the flat case d, where uxx - ux^2 cancels).
The observed distances go to the fixture's `meta`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import _nvs_metrics_oracle as NO

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nvs_metrics.npz")
EVAL = dict(a=(31, 50), b=(20, 33), c=(9, 9), d=(30, 58), e=(31, 50), g=(192, 640), m=(31, 50))
CROP = dict(a=(27, 44), b=(18, 29), c=(7, 7), d=(26, 52), e=(27, 44), g=(172, 576), m=(27, 44))
MUTANT_CASES = dict(cov_norm=("a", "b", "c", "g"), margin=("a", "b", "g"), box=("a", "b", "g"), fp32=("a", "b", "c", "d", "g"))


def smooth(H, W, phase):
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ch = np.arange(3, dtype=np.float64)
    return 0.5 + 0.35 * np.sin(0.31 * xx[..., None] + 0.9 * ch + phase) * np.cos(0.23 * yy[..., None] - 0.5 * ch)


def inputs(name):
    """(pred, gt), float32 (H, W, 3); for m: (3, H, W, 3) each"""
    rng = np.random.default_rng(dict(a=1, b=2, c=3, d=4, e=1, m=1)[name]) if name != "g" else None
    if name in ("a", "e", "m"):
        gt = smooth(24, 40, 0.0)
        pred = np.clip(gt + 0.08 * rng.standard_normal(gt.shape), 0, 1)
        if name == "e":
            pred = gt
        if name == "m":
            gts = [gt, smooth(24, 40, 1.3), rng.random(gt.shape)]
            preds = [pred, np.clip(gts[1] + 0.02 * rng.standard_normal(gt.shape), 0, 1), rng.random(gt.shape)]
            return np.stack(preds).astype(np.float32), np.stack(gts).astype(np.float32)
    elif name == "b":
        gt = np.clip(smooth(48, 70, 0.4) + 0.05 * rng.standard_normal((48, 70, 3)), 0, 1)
        pred = np.clip(smooth(48, 70, 0.5) + 0.05 * rng.standard_normal((48, 70, 3)), 0, 1)
    elif name == "c":
        pred, gt = rng.random((9, 9, 3)), rng.random((9, 9, 3))
    elif name == "d":
        pred, gt = 0.5 + 1e-3 * (2 * rng.random((30, 58, 3)) - 1), 0.5 + 1e-3 * (2 * rng.random((30, 58, 3)) - 1)
    elif name == "g":
        return NO.inputs_g()
    return pred.astype(np.float32), gt.astype(np.float32)


def check_case(name, pred, gt, meta):
    res = EVAL[name]
    row = NO.evaluate(pred, gt, res)
    y0, y1, x0, x1 = NO.crop_box(*res)
    assert (y1 - y0, x1 - x0) == CROP[name], (name, y1 - y0, x1 - x0)
    assert row[6] == (y1 - y0 - 6) * (x1 - x0 - 6) and row[7] == (y1 - y0) * (x1 - x0)
    direct = NO.evaluate_direct(pred, gt, res)
    d_ssim = float(np.max(np.abs(row[[0, 3, 4, 5]] - direct[[0, 3, 4, 5]])))
    d_mse = float(abs(row[2] - direct[2]) / row[2]) if row[2] else float(direct[2])
    assert d_ssim <= 1e-13 and d_mse <= 1e-14, (name, d_ssim, d_mse)
    assert row[6] == direct[6] and row[7] == direct[7]
    m = dict(direct_ssim=d_ssim, direct_mse_rel=d_mse)
    mutants = dict(cov_norm=dict(cov_norm=1.0), margin=dict(margin=2), box=dict(box=(y0, y1, x0, x1 - 1)), fp32=dict(dtype=np.float32))
    for k, kw in mutants.items():
        if name in MUTANT_CASES[k]:
            m[k] = float(abs(NO.evaluate(pred, gt, res, **kw)[0] - row[0]))
            assert m[k] > (1e-11 if k == "fp32" else 1e-6), (name, k, m[k])
    meta[name] = m
    return row


def generate():
    arrays, meta = {}, {}
    for name in ("a", "b", "c", "d", "e", "g"):
        pred, gt = inputs(name)
        arrays[f"{name}_row"] = check_case(name, pred, gt, meta)
        if name in ("a", "b", "c", "d"):
            arrays[f"{name}_pred"], arrays[f"{name}_gt"] = pred, gt
    assert arrays["c_row"][6] == 1
    assert arrays["e_row"][2] == 0 and np.isposinf(arrays["e_row"][1]) and abs(arrays["e_row"][0] - 1) <= 1e-13
    preds, gts = inputs("m")
    assert np.array_equal(preds[0], arrays["a_pred"]) and np.array_equal(gts[0], arrays["a_gt"])
    arrays["m_pred"], arrays["m_gt"] = preds[1:], gts[1:]           # frame 0 is case a
    rows = [check_case("m", preds[i], gts[i], meta) for i in range(3)]
    assert np.array_equal(rows[0], arrays["a_row"])
    arrays["m_rows"] = np.stack(rows)
    arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return arrays


if __name__ == "__main__":
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(json.dumps(json.loads(str(arrays["meta"])), indent=1))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
