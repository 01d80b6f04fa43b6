"""Golden fixture for the depth evaluation metrics FROM THE REAL REFERENCE.  Run in the build container only:

    python -B tests/golden/gen_golden_depth_metrics.py

Imports the reference's models/bts/evaluator.py unmodified (its third-party imports -- ignite, lpips, skimage, the dataset factory, the
evaluation driver, the metric class -- are stubbed here before the import; oracle/ref_shim.py supplies the rest) and calls
BTSWrapper.compute_depth_metrics on a bare object that carries only `depth_scaling`, on the CPU, in fp32 and, as the arbiter, with
every input cast to fp64.  torch.median and torch.linalg.lstsq are wrapped while the reference runs, so that the medians and the
coefficients it computed are recorded too.  Nothing of the reference's source enters the repository; the inputs and outputs do:
tests/golden/depth_metrics.npz.

Seeded cases (pred -> gt, mode):
  a  26 x 30 -> 44 x 58, median: resize indices where the fp32 formula and the exact rational differ (asserted, per axis); about 40 %
     valid pixels, N odd; gt quantised to 1/256 m (ties asserted)
  b  24 x 80 -> 47 x 155, median: dense gt, N even with two different middle elements in gt and in pred; pred in [10, 10.01] so that
     keys share their upper 22 bits (asserted: the bin of the wanted rank holds more than one distinct key after the second radix
     pass); scaled values on both sides of the clamp's upper bound and below its lower bound
  c  a's inputs, l2          d  a's inputs, no scaling (the evaluator_nvs.py form)
  e  a with three negative gt pixels, median: the two masks differ, rmse_log is NaN
  f  3 frames of a's size from other seeds, median

The generator ASSERTS the bars of tests/test_gpu_depth_metrics.py on the fp32 reference itself, against the fp64 sum of the
restatement's fp32 terms (tests/_depth_metrics_oracle.py): 2e-6 relative for abs_rel, sq_rel and rmse, 3e-6 + 2e-6 relative for
rmse_log, a1 .. a3 equal to count / N in fp32."""
import json
import math
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from oracle import ref_shim
import _depth_metrics_oracle as DO

OUT = os.path.join(HERE, "depth_metrics.npz")
REL_BAR, LOG_ABS_BAR = 2e-6, 3e-6
SIZE_A, SIZE_B = ((26, 30), (44, 58)), ((24, 80), (47, 155))
MODES = dict(a="median", b="median", c="l2", d=None, e="median", f="median")


def load_evaluator():
    """the reference's evaluator module, imported unmodified"""
    ref_shim.load_reference()

    def stub(name, **attrs):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
        return sys.modules[name]
    ig = stub("ignite")
    ig.contrib = stub("ignite.contrib")
    ig.contrib.handlers = stub("ignite.contrib.handlers", TensorboardLogger=object)
    ig.engine = stub("ignite.engine", Engine=object)
    sk = stub("skimage")
    sk.metrics = stub("skimage.metrics")
    stub("datasets.data_util", make_test_dataset=None)
    stub("utils.base_evaluator", base_evaluation=None)
    stub("utils.metrics", MeanMetric=object)
    import models.bts.evaluator as ev
    return ev


def reference_run(ev, pred, gt, mode):
    """BTSWrapper.compute_depth_metrics on (1, 1, H, W) / (1, 1, Hg, Wg); -> the seven metrics, the medians and the lstsq solution seen"""
    seen = dict(median=[], lstsq=[])
    median, lstsq = torch.median, torch.linalg.lstsq

    def rec_median(x):
        r = median(x)
        seen["median"].append(r.clone())
        return r

    def rec_lstsq(A, b):
        r = lstsq(A, b)
        seen["lstsq"].append(r.solution.squeeze().clone())
        return r
    torch.median, torch.linalg.lstsq = rec_median, rec_lstsq
    try:
        out = ev.BTSWrapper.compute_depth_metrics(types.SimpleNamespace(depth_scaling=mode), dict(depths=[gt], fine=[dict(depth=pred)]))
    finally:
        torch.median, torch.linalg.lstsq = median, lstsq
    return out, seen


def quantise(x):
    return torch.round(x * 256) / 256


def inputs_a(seed):
    (H, W), (Hg, Wg) = SIZE_A
    g = torch.Generator().manual_seed(seed)
    pred = (5 + 35 * torch.rand(H, W, generator=g)).float()
    gt = DO.resize_nearest(pred, Hg, Wg) * 1.2 + 1.5 + 0.3 * torch.randn(Hg, Wg, generator=g)
    off = torch.rand(Hg, Wg, generator=g) < 0.3          # three pixels in ten are off by a factor of up to 2.5, either way
    gt = quantise(torch.where(off, gt * torch.exp(0.92 * (2 * torch.rand(Hg, Wg, generator=g) - 1)), gt))
    valid = torch.rand(Hg, Wg, generator=g) < 0.4
    if int(valid.sum()) % 2 == 0:
        valid.view(-1)[int(valid.view(-1).nonzero()[0])] = False
    gt = torch.where(valid, gt, torch.zeros_like(gt))
    assert int((gt > 0).sum()) % 2 == 1 and (gt >= 0).all()
    return pred.contiguous(), gt.contiguous()


def inputs_b(seed):
    """dense gt but one pixel, N even; the two middle elements differ in gt (one half of the valid pixels below 80 m, the other above)
    and in pred (the seed and the dropped pixel are searched until they do: nearest resizing repeats every source value)"""
    (H, W), (Hg, Wg) = SIZE_B
    for s in range(seed, seed + 64):
        g = torch.Generator().manual_seed(s)
        pred = (10 + 0.01 * torch.rand(H, W, generator=g)).float()
        pred.view(-1)[[3, 500, 1200]] = 1e-5                 # scaled: below the clamp's lower bound
        pr = DO.resize_nearest(pred, Hg, Wg).reshape(-1)
        n = pr.numel() - 1
        assert n % 2 == 0
        for drop in (int(pr.argmin()), int(pr.argmax())):
            keep = torch.ones(pr.numel(), dtype=torch.bool)
            keep[drop] = False
            sp = torch.sort(pr[keep])[0]
            if sp[n // 2 - 1] == sp[n // 2]:
                continue
            order = torch.randperm(n, generator=g)
            far = 4 * torch.randn(n, generator=g).abs() + 1 / 256
            vals = torch.empty(n)
            vals[order[:n // 2]] = quantise(80 - far[:n // 2])
            vals[order[n // 2:]] = quantise(80 + far[n // 2:])
            gt = torch.zeros(pr.numel())
            gt[keep] = vals
            gt = gt.view(Hg, Wg).float()
            sg = torch.sort(gt[gt > 0])[0]
            assert sg.numel() == n and sg[n // 2 - 1] < sg[n // 2]
            return pred.contiguous(), gt.contiguous()
    raise AssertionError("no even-N variant with distinct middle elements")


def keys(x):
    """the ordered bit pattern the radix selection works on"""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(u >= 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)


def check_resize_indices():
    for (H, W), (Hg, Wg) in (SIZE_A,):
        for out, inp in ((Hg, H), (Wg, W)):
            assert (DO.nearest_index(out, inp) != DO.exact_index(out, inp)).any(), (out, inp)


def make_case(ev, name, pred, gt, mode):
    p4, g4 = pred.view(1, 1, *pred.shape), gt.view(1, 1, *gt.shape)
    out32, seen32 = reference_run(ev, p4, g4, mode)
    out64, seen64 = reference_run(ev, p4.double(), g4.double(), mode)
    # (LAPACK's fp32 least squares is not reproducible to the bit -- its result moves with the alignment of its operands -- so the
    # restatement is pinned with the coefficients the reference's own call returned)
    r = DO.evaluate(p4, g4, mode, coeffs=seen32["lstsq"][0].tolist() if mode == "l2" else None)
    m32 = np.array([float(out32[k]) for k in DO.METRIC_KEYS], dtype=np.float32)
    m64 = np.array([float(out64[k]) for k in DO.METRIC_KEYS], dtype=np.float64)
    counts = np.array(r["counts"], dtype=np.int32)
    n = int(counts[0])
    # the restatement IS the reference, bit for bit
    for k in DO.METRIC_KEYS:
        assert torch.equal(r["metrics"][k], out32[k]) or (torch.isnan(r["metrics"][k]) and torch.isnan(out32[k])), (name, k)
    # the bars, on the fp32 reference itself
    want = DO.metrics_from_terms64(r["terms"], r["counts"])
    for i, k in enumerate(DO.METRIC_KEYS):
        a, b = float(m32[i]), want[i]
        if math.isnan(b):
            assert math.isnan(a) and name == "e" and k == "rmse_log", (name, k)
        elif k in ("a1", "a2", "a3"):
            assert a == float(np.float32(counts[2 + i - 4]) / np.float32(n)), (name, k)
        else:
            bar = REL_BAR * abs(b) + (LOG_ABS_BAR if k == "rmse_log" else 0.0)
            assert abs(a - b) <= bar, (name, k, a, b)
    scale = np.array([float(r["scale"]), float(r["shift"])], dtype=np.float32)
    extra, meta = {}, {}
    if mode == "median":
        med_g, med_p = seen32["median"]
        assert float(med_g / med_p) == float(scale[0])
        extra[f"{name}_medians"] = np.array([float(med_g), float(med_p)], dtype=np.float32)
        # the LOWER median
        mask = gt > 0
        sg = torch.sort(gt[mask])[0]
        assert float(med_g) == float(sg[(sg.numel() - 1) // 2])
    if mode == "l2":
        x32 = seen32["lstsq"][0]
        assert float(x32[0]) == float(scale[0]) and float(x32[1]) == float(scale[1])
        mask = gt > 0
        pr = DO.resize_nearest(pred, *gt.shape)[mask].double()
        A = torch.stack((pr, torch.ones_like(pr)), dim=-1)
        x64 = torch.linalg.lstsq(A, gt[mask].double().unsqueeze(-1)).solution.squeeze()      # the arbiter: the same system in fp64
        extra[f"{name}_x64"] = x64.numpy()
        meta["fp32_lstsq_rel_distance_from_fp64"] = [float(abs(x32[i].double() - x64[i]) / abs(x64[i])) for i in range(2)]
        assert float(x64[1].abs()) > 0.1                 # a relative bar on the shift needs a shift away from zero
    print(f"case {name}: mode={mode} counts={counts.tolist()} scale={scale.tolist()} fp32={np.round(m32, 6).tolist()} "
          f"max rel fp32-fp64 {np.nanmax(np.abs(m32 - m64) / np.abs(m64)):.1e} {meta}")
    out = {f"{name}_metrics32": m32, f"{name}_metrics64": m64, f"{name}_counts": counts, f"{name}_scale32": scale}
    out.update(extra)
    return out, meta


def generate():
    ev = load_evaluator()
    check_resize_indices()
    pred_a, gt_a = inputs_a(11)
    pred_b, gt_b = inputs_b(22)
    n_a = int((gt_a > 0).sum())
    assert torch.unique(gt_a[gt_a > 0]).numel() < n_a                                  # ties
    # case b: after two radix passes the bin of the wanted rank still holds several distinct keys; both sides of the clamp are met
    mb = gt_b > 0
    kp = keys(DO.resize_nearest(pred_b, *gt_b.shape)[mb])
    med_key = torch.sort(kp)[0][(kp.numel() - 1) // 2]
    assert torch.unique(kp[(kp >> 10) == (med_key >> 10)]).numel() > 1
    rb = DO.evaluate(pred_b.view(1, 1, *pred_b.shape), gt_b.view(1, 1, *gt_b.shape), "median")
    scaled = float(rb["scale"]) * DO.resize_nearest(pred_b, *gt_b.shape)
    assert (scaled > 80).any() and (scaled < 80).any() and (scaled < 1e-3).any()
    assert int(mb.sum()) % 2 == 0 and int(mb.sum()) == gt_b.numel() - 1
    gt_e = gt_a.clone()
    gt_e.view(-1)[(gt_a.view(-1) == 0).nonzero()[[5, 400, 1100], 0]] = torch.tensor([-5.0, -0.5, -37.25])
    assert int((gt_e < 0).sum()) == 3 and int((gt_e > 0).sum()) == n_a
    frames = [inputs_a(s) for s in (31, 32, 33)]
    pred_f, gt_f = torch.stack([p for p, _ in frames]), torch.stack([g for _, g in frames])

    arrays = dict(a_pred=pred_a, a_gt=gt_a, b_pred=pred_b, b_gt=gt_b, e_gt=gt_e, f_pred=pred_f, f_gt=gt_f)
    out = {k: v.numpy() for k, v in arrays.items()}
    meta = dict(modes={k: str(v) for k, v in MODES.items()}, inputs=dict(c="a", d="a", e="a_pred + e_gt"))
    for name, (pred, gt) in dict(a=(pred_a, gt_a), b=(pred_b, gt_b), c=(pred_a, gt_a), d=(pred_a, gt_a), e=(pred_a, gt_e)).items():
        o, m = make_case(ev, name, pred, gt, MODES[name])
        out.update(o)
        if m:
            meta[name] = m
    per_frame = [make_case(ev, f"f{i}", pred_f[i], gt_f[i], MODES["f"])[0] for i in range(3)]
    for key in ("metrics32", "metrics64", "counts", "scale32", "medians"):
        out[f"f_{key}"] = np.stack([per_frame[i][f"f{i}_{key}"] for i in range(3)])
    assert np.isnan(out["e_metrics32"][3]) and not np.isnan(np.delete(out["e_metrics32"], 3)).any()
    assert out["e_counts"][0] == out["e_counts"][1] + 3
    out["meta"] = np.asarray(json.dumps(meta, sort_keys=True))
    return out


if __name__ == "__main__":
    torch.set_num_threads(4)
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")
