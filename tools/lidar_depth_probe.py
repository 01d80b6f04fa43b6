"""ms per frame of the LiDAR ground-truth depth map (load_depth of the reference's two KITTI data sets) at the evaluation's size: one
synthetic Velodyne sweep of 120 000 points into 375 x 1242, both conventions.  Times, in ONE process,

  library        behindthescenes_amd.load_depth: the clear, the points pass, the pixels pass (fp32 P; kitti_360 also with an fp64 P)
  host_route     the reference's route restated on the host: numpy projection, scatter, Counter over the keys and one np.where per
                 duplicate key, then the upload of the map -- time.perf_counter around both, on the CPU named in the output
  eval_frame_gt  FusedDepthEval.frame with a ready map (192 x 640, K = 64, median scaling)
  frame_lidar    FusedDepthEval.frame_lidar: the same frame with the map formed on the same stream -- the number to report is
                 added_by_lidar = frame_lidar - eval_frame_gt

with HIP events over --iters iterations after --warmup warm-ups; the two frames are alternated in four blocks.  Asserts that library and
host route give maps that are equal in occupancy.  Prints ONE JSON line and, with --out, writes the same numbers as text.

    python tools/lidar_depth_probe.py [--out profiles/<tag>/lidar_depth.txt]"""
import argparse
import json
import math
import os
import platform
import sys
import time
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from behindthescenes_amd import synthetic  # noqa: E402
from tests import _lidar_depth_oracle as LD  # noqa: E402

H, W, HG, WG, C, HD, K, N = 192, 640, 375, 1242, 64, 64, 64, 120000


def cloud(seed=11):
    """a ring-shaped sweep: 360 degrees of azimuth, 26 degrees of elevation, 3 .. 70 m"""
    rng = np.random.default_rng(seed)
    ang, r = rng.uniform(-math.pi, math.pi, N), rng.uniform(3.0, 70.0, N)
    elev = np.radians(rng.uniform(-24.0, 2.0, N))
    pts = np.stack([r * np.cos(ang), r * np.sin(ang), r * np.tan(elev) + 0.1, rng.uniform(0, 1, N)], axis=1)
    return np.ascontiguousarray(pts.astype(np.float32))


def projection(convention):
    """velodyne (x forward, y left, z up) -> camera, KITTI's intrinsics in pixels (kitti_raw) or normalised to [-1, 1] (kitti_360)"""
    Rt = np.array([[0.0, -1, 0, 0.0], [0, 0, -1, -0.08], [1, 0, 0, -0.27]])
    if convention == "kitti_raw":
        Kc = np.array([[721.5, 0, 609.6], [0, 721.5, 172.9], [0, 0, 1]])
    else:
        Kc = np.array([[1.16, 0, -0.02], [0, 3.84, -0.08], [0, 0, 1]])
    return Kc @ Rt


def host_load_depth(points, P, size, convention):
    """the reference's function restated with numpy and a Counter (rules 1 - 7 of include/bts_render.h in its order and with its loop)"""
    Hh, Ww = size
    idx, x, y, z = LD.project(points, P, size, convention)
    depth = np.zeros(size)
    depth[y, x] = z
    keys = y * (Ww - 1) + x - 1
    for key in [k for k, c in Counter(keys.tolist()).items() if c > 1]:
        members = np.where(keys == key)[0]
        depth[y[members[0]], x[members[0]]] = z[members].min()
    depth[depth < 0] = 0
    return depth[None]


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


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def frame_setup():
    scene = synthetic.synthetic_scene(1, 2, H, W, C, seed=9, intrinsics=synthetic.K_KITTIRAW, smooth=True)
    torch.manual_seed(4)
    net = bts.BTSNet(synthetic.field_conf(C, HD, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), C, num_views=1)
    synthetic.init_mlp_(net.mlp_coarse, seed=7)
    net = net.cuda().eval()
    wrapped = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=True)).bind_parallel(net).eval().cuda()
    return wrapped, bts.ImageRaySampler(3.0, 80.0), [scene[k].cuda() for k in ("images", "projs", "poses")]


def run(iters, warmup):
    out = dict(metric="ms_per_frame", points=N, size=[HG, WG], iters=iters, warmup=warmup, host_cpu=cpu_name(),
               host_threads=torch.get_num_threads())
    pts = cloud()
    pts_dev = torch.from_numpy(pts).cuda()
    size = (HG, WG)
    for convention in LD.CONVENTIONS:
        P = projection(convention)
        variants = [("fp32", P.astype(np.float32))] + ([("fp64", P)] if convention == "kitti_360" else [])
        for tag, Pv in variants:
            P_dev = torch.from_numpy(np.ascontiguousarray(Pv)).cuda()
            out[f"{convention}_library_{tag}"] = round(mean_ms(lambda: bts.load_depth(pts_dev, P_dev, size, convention), iters, warmup), 4)
            mine = bts.load_depth(pts_dev, P_dev, size, convention).cpu().numpy()
            t = []
            for _ in range(5):
                t0 = time.perf_counter()
                host = host_load_depth(pts, Pv, size, convention)
                up = torch.from_numpy(host).cuda()
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            out[f"{convention}_host_route_{tag}"] = round(sorted(t)[2], 3)
            assert np.array_equal(mine != 0, host != 0), (convention, tag)
            assert np.array_equal(mine.astype(np.float64) != 0, up.cpu().numpy() != 0)
            out[f"{convention}_occupied_{tag}"] = int((host != 0).sum())
    wrapped, sampler, frame_inputs = frame_setup()
    jitter = torch.rand(2 * H * W, K, device="cuda")
    kw = dict(ids_encoder=[0], ids_render=[0], jitter=jitter)
    for convention in LD.CONVENTIONS:
        P_dev = torch.from_numpy(np.ascontiguousarray(projection(convention).astype(np.float32))).cuda()
        gt = bts.load_depth(pts_dev, P_dev, size, convention)
        ev = bts.FusedDepthEval(wrapped, sampler, depth_scaling="median", capacity=iters + warmup + 8)
        t_gt, t_lidar = [], []
        for _ in range(4):                     # alternated in blocks, so that a drifting clock meets both
            ev.reset()
            t_gt.append(mean_ms(lambda: ev.frame(*frame_inputs, gt, **kw), iters // 4, warmup // 4 + 1))
            ev.reset()
            t_lidar.append(mean_ms(lambda: ev.frame_lidar(*frame_inputs, pts_dev, P_dev, convention, size=size, **kw), iters // 4, warmup // 4 + 1))
        out[f"{convention}_eval_frame_gt"] = round(sum(t_gt) / 4, 4)
        out[f"{convention}_frame_lidar"] = round(sum(t_lidar) / 4, 4)
        out[f"{convention}_added_by_lidar"] = round(out[f"{convention}_frame_lidar"] - out[f"{convention}_eval_frame_gt"], 4)
        out[f"{convention}_eval_frame_gt_blocks"] = [round(t, 4) for t in t_gt]
        out[f"{convention}_frame_lidar_blocks"] = [round(t, 4) for t in t_lidar]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = run(args.iters, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("LiDAR ground-truth depth map, ms per frame (tools/lidar_depth_probe.py; library and frames: HIP events, mean over "
                    f"{res['iters']} iterations after {res['warmup']} warm-ups; host route: time.perf_counter, median of 5, map upload included)\n")
            for k, v in res.items():
                f.write(f"{k:44s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
