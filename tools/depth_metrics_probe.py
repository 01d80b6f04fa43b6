"""ms per frame of the depth evaluation metrics (evaluator.py:96-151) at the benchmarked size: a 192 x 640 prediction against a
375 x 1242 ground truth (KITTI's), median scaling, with 5 % (LiDAR-like) and 100 % valid pixels.  Times, in ONE process,

  library        bts_depth_metrics: the clear, the three radix passes, the metrics pass, finish (mode none: the last two only)
  torch_eager    tests/_depth_metrics_oracle.py, the suite's torch restatement of the reference's function, run eagerly on the GPU with
                 the reference's synchronisations (two boolean-mask gathers, two medians) and the seven .item() calls MeanMetric makes
  eval_frame     FusedEvalFrame alone (bts_eval_frame, 192 x 640, K = 64)
  depth_eval     FusedDepthEval.frame: the same frame + bts_depth_metrics on the same stream -- the number to report is
                 added_by_metrics = depth_eval - eval_frame

with HIP events over --iters iterations after --warmup warm-ups (mean of the timed window).  The kernels of the library call are timed
in a run of their own: --kernels starts `rocprofv3 --kernel-trace --stats` on a child process of this script per valid fraction and
lists the average of every depth_* kernel.  Prints ONE JSON line and, with --out, writes the same numbers as text.

    python tools/depth_metrics_probe.py [--kernels] [--out profiles/<dir>/depth_metrics.txt]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from behindthescenes_amd import native, synthetic  # noqa: E402
from tests import _depth_metrics_oracle as DO  # noqa: E402

H, W, HG, WG, C, HD, K = 192, 640, 375, 1242, 64, 64, 64
FRACTIONS = (0.05, 1.0)


def inputs(fraction, dev="cuda"):
    g = torch.Generator().manual_seed(5)
    pred = 3 + 60 * torch.rand(1, 1, H, W, generator=g)
    gt = (DO.resize_nearest(pred, HG, WG) * 1.1 + torch.randn(1, 1, HG, WG, generator=g)).clamp_min(0.5)
    if fraction < 1.0:
        gt = torch.where(torch.rand(1, 1, HG, WG, generator=g) < fraction, gt, torch.zeros(()))
    return pred.to(dev).contiguous(), gt.to(dev).contiguous()


def mean_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def frame_setup():
    scene = synthetic.synthetic_scene(1, 2, H, W, C, seed=9, intrinsics=synthetic.K_KITTIRAW, smooth=True)
    torch.manual_seed(4)
    net = bts.BTSNet(synthetic.field_conf(C, HD, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), C, num_views=1)
    synthetic.init_mlp_(net.mlp_coarse, seed=7)
    net = net.cuda().eval()
    wrapped = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=True)).bind_parallel(net).eval().cuda()
    return wrapped, bts.ImageRaySampler(3.0, 80.0), [scene[k].cuda() for k in ("images", "projs", "poses")]


def torch_eager(pred, gt, mode):
    m = DO.evaluate(pred, gt, mode)["metrics"]
    return [m[k].item() for k in DO.METRIC_KEYS]


def run(iters, warmup):
    out = dict(metric="ms_per_frame", pred=[H, W], gt=[HG, WG], iters=iters, warmup=warmup)
    for fraction in FRACTIONS:
        pred, gt = inputs(fraction)
        tag = f"valid_{int(round(fraction * 100))}pct"
        rows = torch.empty((1, 12), device="cuda")
        for mode in ("median", "l2", None):
            out[f"{tag}_library_{mode}"] = round(mean_ms(lambda: native.depth_metrics(pred[0], gt[0], mode, out=rows), iters, warmup), 4)
        out[f"{tag}_torch_eager_median"] = round(mean_ms(lambda: torch_eager(pred, gt, "median"), max(20, iters // 4), max(5, warmup // 5)), 4)
        a = bts.compute_depth_metrics(pred, gt, "median")
        b = torch_eager(pred, gt, "median")
        out[f"{tag}_abs_rel_library_vs_torch"] = [round(a["abs_rel"].item(), 7), round(b[0], 7)]
    wrapped, sampler, frame_inputs = frame_setup()
    pred, gt = inputs(FRACTIONS[0])
    jitter = torch.rand(2 * H * W, K, device="cuda")
    alone = bts.FusedEvalFrame(wrapped, sampler)
    ev = bts.FusedDepthEval(wrapped, sampler, depth_scaling="median", capacity=iters + warmup)

    def with_metrics():
        ev.frame(*frame_inputs, gt, ids_encoder=[0], ids_render=[0], jitter=jitter)
    # the two are alternated in blocks, so that a drifting clock meets both
    t_alone, t_with = [], []
    for _ in range(4):
        ev.reset()
        t_alone.append(mean_ms(lambda: alone(*frame_inputs, ids_encoder=[0], ids_render=[0], jitter=jitter), iters // 4, warmup // 4 + 1))
        t_with.append(mean_ms(with_metrics, iters // 4, warmup // 4 + 1))
    out["eval_frame"] = round(sum(t_alone) / 4, 4)
    out["depth_eval_valid_5pct_median"] = round(sum(t_with) / 4, 4)
    out["added_by_metrics"] = round(out["depth_eval_valid_5pct_median"] - out["eval_frame"], 4)
    out["eval_frame_blocks"], out["depth_eval_blocks"] = [round(t, 4) for t in t_alone], [round(t, 4) for t in t_with]
    return out


def child(fraction, iters):
    """what rocprofv3 traces: the library call alone, median mode"""
    pred, gt = inputs(fraction)
    rows = torch.empty((1, 12), device="cuda")
    for _ in range(iters):
        native.depth_metrics(pred[0], gt[0], "median", out=rows)
    torch.cuda.synchronize()


def kernel_times(iters):
    res = {}
    for fraction in FRACTIONS:
        with tempfile.TemporaryDirectory() as d:
            cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "trace", "--", sys.executable, os.path.abspath(__file__),
                   "--child", str(fraction), "--iters", str(iters)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
            if r.returncode != 0 or not files:
                res[f"valid_{int(round(fraction * 100))}pct"] = f"rocprofv3 failed ({r.returncode}): {r.stderr[-300:]}"
                continue
            rows = [x for x in csv.DictReader(open(files[0])) if "depth_" in x["Name"]]
            res[f"valid_{int(round(fraction * 100))}pct"] = {x["Name"].split("(")[0].replace("void bts::", ""): round(float(x["AverageNs"]) / 1e3, 2)
                                                              for x in rows}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--kernels", action="store_true", help="also time every kernel of the call (rocprofv3 on a child process)")
    ap.add_argument("--child", type=float, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child is not None:
        child(args.child, args.iters)
        sys.exit(0)
    res = run(args.iters, args.warmup)
    if args.kernels:
        res["kernel_average_us"] = kernel_times(args.iters + args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("Depth evaluation metrics, ms per frame (tools/depth_metrics_probe.py; HIP events, mean over "
                    f"{res['iters']} iterations after {res['warmup']} warm-ups; kernel averages in microseconds from rocprofv3 --kernel-trace --stats)\n")
            for k, v in res.items():
                f.write(f"{k:44s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
