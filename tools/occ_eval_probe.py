"""ms per frame of the LiDAR occupancy evaluation after the render (evaluator_lidar.py:292-340) at the real size: 20 clouds of 120 000
points, the 80 x 160 x 1 query grid, a 192 x 640 field.  Times, in ONE process,

  fused     behindthescenes_amd.FusedOccupancyEval: bts_occupancy_eval + the one device-to-host copy of the six counts
  pieces    the same work entry by entry (field query, bts_lidar_slices, bts_invert_small + bts_lidar_occupancy); what remains of the
            fused call (the metrics kernel, the camera inverse, the copy) is reported as the difference
  torch     tests/_lidar_occ_oracle.py, the suite's vectorised torch restatement of the reference's functions, run eagerly on the GPU
            with the density query on the HIP kernel -- the role `ref_gpu_baseline` plays in bench.py.  (The reference's own functions
            loop over 360 bins per cloud in Python and are slower still.)

with HIP events after >= 25 ms of continuous warm-up work, median over --reps repetitions.  Prints ONE JSON line and, with --out,
writes the same numbers as text.

    python tools/occ_eval_probe.py [--reps 20] [--out profiles/r08a/occ_eval.txt]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from behindthescenes_amd import lidar_occupancy as L  # noqa: E402
from behindthescenes_amd import native, synthetic  # noqa: E402
from tests import _lidar_occ_oracle as LO  # noqa: E402

T, N_PTS, H, W, C, HD = 20, 120_000, 192, 640, 64, 64


def _net():
    conf = dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=False, code_mode="z", code=dict(num_freqs=6, freq_factor=1.5, include_input=True),
                encoder=dict(type="feature_map", size=(H, W), d_out=C), mlp_coarse=dict(type="resnet", n_blocks=0, d_hidden=HD),
                mlp_fine=dict(type="empty"))
    g = torch.Generator().manual_seed(0)
    net = bts.BTSNet(conf)
    with torch.no_grad():
        net.encoder.feats[0].data = torch.randn((1, C, H, W), generator=g) * 0.5
        for p in net.mlp_coarse.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if p.dim() > 1 else 0.05))
    net = net.cuda().eval()
    s = synthetic.synthetic_scene(1, 3, H, W, C, seed=0, smooth=True)
    net.encode(s["images"].cuda(), s["projs"].cuda(), s["poses"].cuda(), ids_encoder=[0], ids_render=[1, 2])
    return net, s["projs"][0, 0].cuda().contiguous(), s["poses"][0, 0].cuda().contiguous()


def _clouds():
    """ring-shaped clouds in the velodyne frame (x forward, y left, z up) and their poses into the camera-like world frame"""
    g = torch.Generator(device="cuda").manual_seed(1)
    clouds, poses = [], []
    for k in range(T):
        ang = (torch.rand(N_PTS, device="cuda", generator=g) * 2 - 1) * math.pi
        r = 9 + 4 * torch.sin(3 * ang + 0.3 * k) + torch.randn(N_PTS, device="cuda", generator=g)
        r = torch.where(torch.rand(N_PTS, device="cuda", generator=g) < 0.15, r + 25, r).clamp_min(0.5)
        z = torch.rand(N_PTS, device="cuda", generator=g) * 3 - 2
        clouds.append(torch.stack((r * torch.cos(ang), r * torch.sin(ang), z, torch.ones_like(z)), dim=1).contiguous())
        a = math.radians(0.5 * k)
        poses.append(torch.tensor([[-math.sin(a), -math.cos(a), 0, 0.02 * k], [0, 0, -1, 1.0], [math.cos(a), -math.sin(a), 0, 0.6 * k - 0.5],
                                   [0, 0, 0, 1]], dtype=torch.float32))
    return clouds, torch.stack(poses).cuda()


def _median_ms(fn, reps):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    fn()
    e[1].record()
    e[1].synchronize()
    for _ in range(max(3, int(40.0 / max(e[0].elapsed_time(e[1]), 1e-3)) + 1)):      # >= 25 ms of continuous warm-up work
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def run(reps):
    net, proj, pose = _net()
    clouds, poses = _clouds()
    depth = (6 + 14 * torch.rand((H, W), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))).contiguous()
    ev = bts.FusedOccupancyEval(net)
    q = ev.q_pts(torch.device("cuda", torch.cuda.current_device()))
    y_range, max_dist = ev.y_range, ev.max_dist

    def fused():
        return ev(clouds, poses, depth, proj, pose)

    def query():
        with torch.no_grad():
            return net(q.unsqueeze(0), only_density=True)[2]
    tables = L.lidar_tables(clouds, poses, y_range, 1, max_dist)

    def torch_eager():
        with torch.no_grad():
            sigma = net(q.unsqueeze(0), only_density=True)[2].reshape(-1)
            tab = LO.lidar_tables(clouds, poses, y_range, 1, max_dist)
            occ, vis = LO.check_occupancy(q, tab, poses, ev.min_dist)
            dist, pred, _ = LO.predicted_visibility(q, proj, pose, depth)
            return LO.metrics(occ, vis, dist <= pred, sigma > ev.occ_threshold)[0]

    out = dict(metric="ms_per_frame", clouds=T, points_per_cloud=N_PTS, query_points=int(q.shape[0]), reps=reps)
    out["fused"] = round(_median_ms(fused, reps), 4)
    out["field_query"] = round(_median_ms(query, reps), 4)
    out["lidar_slices"] = round(_median_ms(lambda: L.lidar_tables(clouds, poses, y_range, 1, max_dist), reps), 4)
    out["lidar_occupancy"] = round(_median_ms(lambda: L.occupancy_masks(q, tables, native.invert_small(poses), ev.min_dist), reps), 4)
    out["metrics_inverse_copy_by_difference"] = round(out["fused"] - out["field_query"] - out["lidar_slices"] - out["lidar_occupancy"], 4)
    out["torch_eager_restatement"] = round(_median_ms(torch_eager, max(3, reps // 4)), 4)
    # the two paths agree (the restatement is the suite's yardstick; random clouds have no decision margins, so a few points may differ)
    a, b = fused(), torch_eager()
    out["o_acc_fused_vs_torch"] = [round(float(a["o_acc"]), 6), round(float(b["o_acc"]), 6)]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = run(max(20, args.reps))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("LiDAR occupancy evaluation after the render, ms per frame (tools/occ_eval_probe.py; HIP events, median of "
                    f"{res['reps']} repetitions after >= 25 ms of warm-up)\n")
            for k, v in res.items():
                f.write(f"{k:40s} {v}\n")
