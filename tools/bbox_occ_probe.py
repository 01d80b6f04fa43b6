"""ms per frame of the 3D-bounding-box occupancy evaluation around the render (evaluator_3dbb.py:201-241, :253-299) at the real size: a
192 x 640 frame (96 x 320 rays under a 192 x 640 label map), 50 boxes of 8 vertices / 12 triangles, the 13 600 query points.  Times, in
ONE process,

  fused     behindthescenes_amd.FusedBBoxOccupancyEval: bts_bbox_occupancy_eval + the one device-to-host copy of the seven integers
  pieces    the same work entry by entry (field query, bts_invert_small + bts_bbox_bounds, bts_bbox_pseudo_depth); what remains of the
            fused call (the metrics kernel, the copy) is reported as the difference
  torch     tests/_bbox_occ_oracle.py, the suite's torch restatement of the reference's sequence (box by box: bounds, frustum test,
            labelled intercepts, in_bbox; two grid_sample look-ups; the reductions), run eagerly on the same GPU with the density query
            on the HIP kernel

with HIP events over --iters iterations after --warmup warm-ups (mean of the timed window).  The fused call and the eager restatement
are alternated in blocks, so that a drifting clock meets both.  Prints ONE JSON line and, with --out, writes the same numbers as text.

    python tools/bbox_occ_probe.py [--out profiles/r12a/bbox_occ.txt]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import behindthescenes_amd as bts  # noqa: E402
from behindthescenes_amd import bbox_occupancy as BB  # noqa: E402
from behindthescenes_amd import synthetic  # noqa: E402
from oracle import bts_oracle as O  # noqa: E402
from tests import _bbox_occ_oracle as BO  # noqa: E402

H, W, C, HD, N_BOXES = 192, 640, 64, 64, 50
PH, PW = H // 2, W // 2
LABELS = (24.0, 26.0, 27.0, 28.0, 33.0)
QUADS = ((0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5))


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
    return net, s["projs"][0, 0].contiguous()


def _boxes(pose):
    """50 yawed cuboids over the query volume as the data loader hands them over: world vertices (1, 8, 3), faces (1, 12, 3), semanticId"""
    g = torch.Generator().manual_seed(3)
    faces = torch.tensor([t for a, b, c, d in QUADS for t in ((a, b, c), (a, c, d))], dtype=torch.int64)
    corners = torch.tensor([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=torch.float32)
    out = []
    for k in range(N_BOXES):
        u = torch.rand(6, generator=g)
        z = 4 + 20 * float(u[0])
        centre = torch.tensor([-5 + 10 * float(u[1]), 0.5 - 0.0875 * z, z])
        a = math.radians(180 * float(u[2]))
        rot = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        v = (corners * torch.tensor([0.8 + 0.4 * float(u[3]), 0.8, 1.6 + float(u[4])])) @ rot.T + centre
        v = (pose[:3, :3] @ v.T + pose[:3, 3, None]).T
        out.append(dict(vertices=v[None].contiguous().cuda(), faces=faces[None].cuda(), semanticId=torch.tensor(int(LABELS[k % len(LABELS)]))))
    return out


def run(iters, warmup):
    net, proj_cpu = _net()
    pose_cpu = O._pose(tx=0.05, ty=-0.03, tz=0.1, yaw_deg=2.0)
    proj, pose = proj_cpu.cuda(), pose_cpu.cuda()
    boxes = _boxes(pose_cpu)
    g = torch.Generator().manual_seed(4)
    seg = torch.tensor(LABELS + (0.0,))[torch.randint(len(LABELS) + 1, (H, W), generator=g)].cuda().contiguous()
    rays = O.image_rays(torch.eye(4).view(1, 1, 4, 4), proj_cpu.view(1, 1, 3, 3), PH, PW, 3.0, 80.0)[0].cuda().contiguous()
    depth = (4 + 10 * torch.rand((PH, PW), generator=g)).cuda().contiguous()
    ev = bts.FusedBBoxOccupancyEval(net)
    q = ev.q_pts(torch.device("cuda", torch.cuda.current_device()))
    packed = BB.pack_bboxes(boxes)
    verts, faces, labels = [b["vertices"][0] for b in boxes], [b["faces"][0] for b in boxes], [float(b["semanticId"]) for b in boxes]

    def fused():
        return ev(packed, seg, rays, (PH, PW), depth, proj, pose)

    def fused_with_packing():
        return ev(boxes, seg, rays, (PH, PW), depth, proj, pose)

    def query():
        with torch.no_grad():
            return net(q.unsqueeze(0), only_density=True)[2]

    def tables():
        return BB.bbox_tables(packed[0], packed[1], packed[3], packed[4], pose, proj, ev.max_d)
    tab = tables()

    def torch_eager():
        with torch.no_grad():
            sigma = net(q.unsqueeze(0), only_density=True)[2].reshape(-1)
            return BO.eager_frame(verts, faces, labels, pose, proj, ev.max_d, rays[:, 3:6], seg, (PH, PW), depth, q, sigma, ev.occ_threshold)

    out = dict(metric="ms_per_frame", frame=[H, W], rays=PH * PW, boxes=N_BOXES, query_points=int(q.shape[0]), iters=iters, warmup=warmup)
    t_fused, t_torch = [], []
    for _ in range(4):
        t_fused.append(mean_ms(fused, iters // 4, warmup // 4 + 1))
        t_torch.append(mean_ms(torch_eager, max(3, iters // 40), 2))
    out["fused"], out["torch_eager_restatement"] = round(sum(t_fused) / 4, 4), round(sum(t_torch) / 4, 4)
    out["fused_blocks"], out["torch_eager_blocks"] = [round(t, 4) for t in t_fused], [round(t, 4) for t in t_torch]
    out["fused_with_pack_bboxes"] = round(mean_ms(fused_with_packing, iters // 4, warmup // 4 + 1), 4)
    out["field_query"] = round(mean_ms(query, iters, warmup), 4)
    out["bbox_bounds_with_inverse"] = round(mean_ms(tables, iters, warmup), 4)
    out["bbox_pseudo_depth"] = round(mean_ms(lambda: BB.pseudo_depth(rays, (PH, PW), seg, tab[0], tab[1], tab[2], packed[2]), iters, warmup), 4)
    out["metrics_copy_by_difference"] = round(out["fused"] - out["field_query"] - out["bbox_bounds_with_inverse"] - out["bbox_pseudo_depth"], 4)
    # the two paths agree (random boxes have no decision margins, so a few points may differ)
    a, (b, pd) = fused(), torch_eager()
    out["active_boxes"], out["finite_pseudo_depth_rays"] = a["counts"][6], int(torch.isfinite(pd).sum())
    out["counts_fused_vs_torch"] = [a["counts"][:6], b]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bbox_occ_probe: no GPU; nothing is measured without one")
    res = run(args.iters, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("3D-bounding-box occupancy evaluation, ms per frame (tools/bbox_occ_probe.py; HIP events, mean over "
                    f"{res['iters']} iterations after {res['warmup']} warm-ups, fused and eager alternated in four blocks)\n")
            for k, v in res.items():
                f.write(f"{k:40s} {json.dumps(v) if isinstance(v, (dict, list)) else v}\n")
