"""Golden fixture for the LiDAR occupancy evaluation FROM THE REAL REFERENCE.  Run in the build container only:

    python -B tests/golden/gen_golden_lidar_occ.py

Imports the reference's models/bts/evaluator_lidar.py unmodified (its third-party imports -- ignite, the dataset factory, the evaluation
driver, the metric class -- are stubbed here before the import; oracle/ref_shim.py supplies the rest) and runs its get_pts,
get_lidar_slices, check_occupancy, project_into_cam and the metric statements of BTSWrapper.forward (cut out of the source as AST nodes
and executed unmodified) on the CPU, in fp32 and, for arbitration, in fp64.  Nothing of the reference's source enters the repository;
the inputs and outputs do: tests/golden/lidar_occ.npz.

Two seeded synthetic cases.  A: the evaluator's settings (y_res = 1, 80 x 160 grid), T = 4 ring-shaped clouds of 3 000 points with
empty leading and interior bins, points beyond max_dist, a pose per cloud.  B: y_res = 3, P not a multiple of 3, T = 3 (thresh = 1/3).
The generator ASSERTS, in fp64, that the fp32 reference is itself unambiguous on the scene (angles away from bin borders, heights away
from slice bounds, norms away from max_dist, a unique smallest angle) and stores a per-point `decided` mask: points all of whose
comparisons are clear of their thresholds by the margins below.  Undecided points are capped at 1 % of P."""
import ast
import math
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import torch.nn.functional as F

from oracle import bts_oracle as O
from oracle import ref_shim
import _lidar_occ_oracle as LO

OUT = os.path.join(HERE, "lidar_occ.npz")
ANGLE_MARGIN, Y_MARGIN, NORM_MARGIN, FIRST_MARGIN = 1e-4, 1e-4, 1e-3, 1e-4
SURFACE_REL, MIN_DIST_ABS, PRED_REL, TIE_PX, SIGMA_ABS = 1e-4, 1e-4, 1e-5, 1e-3, 1e-3
X_RANGE, Y_RANGE, Z_RANGE = (-4, 4), (0, .75), (20, 4)
MAX_DIST = (Z_RANGE[0] ** 2 + X_RANGE[0] ** 2) ** .5
MIN_DIST, OCC_THRESHOLD = 3, 0.5
NET = dict(seed=5, H=48, W=160, C=64, Hd=64, v=3, b_out=1.2)   # the encoded net of the fused call's test, rebuilt there from the seed
METRIC_KEYS = ("o_acc", "o_rec", "o_prec", "ie_acc", "ie_rec", "ie_prec", "ie_r", "t_ie", "t_no_nop_nv")


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
    stub("datasets.data_util", make_test_dataset=None)
    stub("utils.base_evaluator", base_evaluation=None)
    stub("utils.metrics", MeanMetric=object)
    import matplotlib
    matplotlib.use("Agg")
    import models.bts.evaluator_lidar as ev
    return ev


def forward_statements(ev):
    """Code objects cut out of BTSWrapper.forward, unmodified: the depth look-up (`pred_dist = ...`) and the statements from
    `is_visible |= is_visible_pred` to the last metric."""
    path = ev.__file__
    tree = ast.parse(open(path).read())
    fwd = next(f for c in tree.body if isinstance(c, ast.ClassDef) and c.name == "BTSWrapper"
               for f in c.body if isinstance(f, ast.FunctionDef) and f.name == "forward")

    def assigns(name):
        return next(i for i, s in enumerate(fwd.body) if isinstance(s, ast.Assign) and getattr(s.targets[0], "id", "") == name)
    first = next(i for i, s in enumerate(fwd.body) if isinstance(s, ast.AugAssign) and getattr(s.target, "id", "") == "is_visible")
    lookup = fwd.body[assigns("pred_dist")]
    return (compile(ast.Module(body=[lookup], type_ignores=[]), path, "exec"),
            compile(ast.Module(body=fwd.body[first:assigns("total_no_nop_nv") + 1], type_ignores=[]), path, "exec"))


def run_metrics(code, is_occupied, is_visible, is_visible_pred, is_occupied_pred):
    ns = dict(torch=torch, is_occupied=is_occupied.clone(), is_visible=is_visible.clone(), is_visible_pred=is_visible_pred,
              is_occupied_pred=is_occupied_pred)
    exec(code, ns)
    names = dict(o_acc="is_occupied_acc", o_rec="is_occupied_rec", o_prec="is_occupied_prec", ie_acc="ie_acc", ie_rec="ie_rec", ie_prec="ie_prec",
                 ie_r="not_occupied_not_visible_ratio", t_ie="total_ie", t_no_nop_nv="total_no_nop_nv")
    return np.array([float(ns[names[k]]) for k in METRIC_KEYS], dtype=np.float64), ns["is_occupied"], ns["is_visible"]


def velo_pose(k, gen):
    """velodyne (x forward, y left, z up) -> world (x right, y down, z forward), a yaw and an offset per cloud"""
    base = torch.tensor([[0., -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], dtype=torch.float64)
    a = math.radians(1.5 * k + 0.7)
    b = math.radians(0.4 * k - 0.3)
    yaw = torch.tensor([[math.cos(a), 0, math.sin(a), 0], [0, 1, 0, 0], [-math.sin(a), 0, math.cos(a), 0], [0, 0, 0, 1]], dtype=torch.float64)
    pitch = torch.tensor([[1, 0, 0, 0], [0, math.cos(b), -math.sin(b), 0], [0, math.sin(b), math.cos(b), 0], [0, 0, 0, 1]], dtype=torch.float64)
    m = yaw @ pitch @ base
    m[:3, 3] = torch.tensor([0.15 * k - 0.2, 0.9 + 0.05 * k, 0.8 * k - 0.5], dtype=torch.float64) + 0.02 * torch.randn(3, generator=gen, dtype=torch.float64)
    return m.float()


def make_cloud(n, k, pose, empty_bins, y_bounds, gen):
    """n points of a ring-shaped cloud that satisfy the fixture's margins (checked in fp64 on the fp32 points)"""
    allowed = torch.tensor([b for b in range(LO.N_BINS) if b not in empty_bins])
    m = 4 * n
    bins = allowed[torch.randint(len(allowed), (m,), generator=gen)]
    u = 0.08 + 0.84 * torch.rand(m, generator=gen, dtype=torch.float64)
    ang = -math.pi + (bins.double() + u) * (2 * math.pi / LO.N_BINS)
    r = (6 + 3.5 * k) + 4 * torch.sin(3 * ang + 1.3 * k) + 2 * torch.cos(7 * ang + 1) + 0.6 * torch.randn(m, generator=gen, dtype=torch.float64)
    kind = torch.rand(m, generator=gen)
    r = torch.where(kind < 0.12, 24 + 20 * torch.rand(m, generator=gen, dtype=torch.float64), r)      # beyond max_dist
    r = torch.where(kind > 0.97, 1 + 2.5 * torch.rand(m, generator=gen, dtype=torch.float64), r)      # close returns
    y_world = -0.7 + 2.2 * torch.rand(m, generator=gen, dtype=torch.float64)
    z = float(pose[1, 3]) - y_world
    pc = torch.stack((r * torch.cos(ang), r * torch.sin(ang), z, torch.ones_like(z)), dim=1).float()
    p64 = pc.double()
    a64 = torch.atan2(p64[:, 1], p64[:, 0])
    borders = torch.linspace(-math.pi, math.pi, LO.N_BINS + 1).double()          # the fp32 borders the reference uses
    ok = (a64.view(-1, 1) - borders.view(1, -1)).abs().min(dim=1)[0] > ANGLE_MARGIN
    w64 = (pose.double() @ p64.T).T
    for b in y_bounds:
        ok &= (w64[:, 1] - b).abs() > Y_MARGIN
    ok &= (torch.norm(w64[:, :3], dim=-1) - MAX_DIST).abs() > NORM_MARGIN
    pc = pc[ok][:n]
    assert pc.shape[0] == n, pc.shape
    return pc.contiguous()


def reference_run(ev, lookup, clouds, poses, q_pts, y_res, proj, cam_pose, depth):
    slices = ev.get_lidar_slices(clouds, poses, Y_RANGE, y_res, MAX_DIST)
    is_occupied, is_visible = ev.check_occupancy(q_pts, slices, poses, MIN_DIST)
    cam_pts, dists = ev.project_into_cam(q_pts, proj, cam_pose)
    ns = dict(F=F, torch=torch, pred_depth=depth, h=depth.shape[0], w=depth.shape[1], cam_pts=cam_pts)
    exec(lookup, ns)          # the reference's own look-up statement
    pred_dist = ns["pred_dist"]
    tables = torch.stack([torch.stack(s) for s in slices])
    return tables, is_occupied, is_visible, dists, pred_dist


def make_case(ev, code, name, *, T, n_pts, y_res, q_pts, empty, seed, sigma_of, proj, depth):
    gen = torch.Generator().manual_seed(seed)
    lo, hi = LO.slice_bounds(Y_RANGE, y_res)
    y_bounds = sorted(set(lo.double().tolist() + hi.double().tolist()))
    poses = torch.stack([velo_pose(k, gen) for k in range(T)])
    clouds = [make_cloud(n_pts, k, poses[k], empty[k], y_bounds, gen) for k in range(T)]
    cam_pose = O._pose(tx=0.05, ty=-0.03, tz=0.1, yaw_deg=2.0)
    P = q_pts.shape[0]
    step = P // y_res

    tables, is_occupied, is_visible, dists, pred_dist = reference_run(ev, code[0], clouds, poses, q_pts, y_res, proj, cam_pose, depth)
    torch.set_default_dtype(torch.float64)
    try:
        t64, occ64, vis64, dists64, pred64 = reference_run(ev, code[0], [c.double() for c in clouds], poses.double(), q_pts.double(), y_res, proj.double(),
                                                            cam_pose.double(), depth.double())
    finally:
        torch.set_default_dtype(torch.float32)

    # ---- the scene's own conditions (fp64): selection counts, a unique smallest angle, bin membership identical in fp32 and fp64
    for k in range(T):
        p64 = clouds[k].double()
        w64 = (poses[k].double() @ p64.T).T
        far = torch.norm(w64[:, :3], dim=-1) >= MAX_DIST
        ang = torch.atan2(p64[:, 1], p64[:, 0])
        assert (math.pi - ang.abs()).min() > ANGLE_MARGIN
        for s in range(y_res):
            sel = ((w64[:, 1] >= lo[s].double()) & (w64[:, 1] <= hi[s].double())) | far
            assert int(sel.sum()) >= 360, (name, k, s, int(sel.sum()))
            a = torch.sort(ang[sel])[0]
            assert a[1] - a[0] > FIRST_MARGIN, (name, k, s)
    assert (tables[..., 0].double() - t64[..., 0]).abs().max() < 1e-6      # (the fp64 run builds fp64 borders)
    rel = ((tables[..., 1].double() - t64[..., 1]).abs() / t64[..., 1]).max().item()
    assert rel < 3e-7, rel
    raw = tables[:, :, 1:-1, 1]
    assert all(len(e) > 0 for e in empty) and (raw[:, :, 1:] == raw[:, :, :-1]).any()      # (carried bins exist)

    # ---- decided points
    decided_lidar = torch.ones(P, dtype=torch.bool)
    for i, (d, s) in enumerate(LO.occupancy_terms(q_pts.double(), t64, poses.double())):
        clear = ((d - s).abs() > SURFACE_REL * d) & ((d - MIN_DIST).abs() > MIN_DIST_ABS)
        decided_lidar[i * step:(i + 1) * step] = clear.all(dim=0)
    _, _, pix = LO.predicted_visibility(q_pts.double(), proj.double(), cam_pose.double(), depth.double())
    frac = pix - torch.floor(pix)
    sigma = sigma_of(q_pts)
    decided_pred = ((dists64 - pred64).abs() > PRED_REL * dists64.abs()) & ((frac - 0.5).abs() > TIE_PX).all(dim=1)
    decided = decided_lidar & decided_pred & ((sigma.double() - OCC_THRESHOLD).abs() > SIGMA_ABS)
    assert int((~decided).sum()) <= P // 100, (name, int((~decided).sum()), P)
    assert torch.equal(is_occupied[decided_lidar], occ64[decided_lidar]) and torch.equal(is_visible[decided_lidar], vis64[decided_lidar])
    vis_pred, vis_pred64 = dists <= pred_dist, dists64 <= pred64
    assert torch.equal(vis_pred[decided], vis_pred64[decided])

    occ_pred = sigma > OCC_THRESHOLD
    values, O_mask, V_mask = run_metrics(code[1], is_occupied, is_visible, vis_pred, occ_pred)
    counts = np.array(LO.cell_counts(occ_pred, O_mask, V_mask), dtype=np.int32)
    # (with T = 3 a point that cloud 0 hides is occupied by that one vote: only the remainder points reach the last two cells)
    assert counts.sum() == P and (counts[:4] > 0).all() and (y_res > 1 or (counts > 0).all()), counts
    offsets = np.cumsum([0] + [c.shape[0] for c in clouds]).astype(np.int32)
    arrays = dict(points=torch.cat(clouds), velo_poses=poses, q_pts=q_pts, tables=tables, is_occupied=is_occupied, is_visible=is_visible,
                  is_visible_pred=vis_pred, sigma=sigma, mask_P=occ_pred, mask_O=O_mask, mask_V=V_mask, decided_lidar=decided_lidar,
                  decided=decided, cam_pose=cam_pose)
    out = {f"{name}_{k}": v.numpy() for k, v in arrays.items()}
    out.update({f"{name}_offsets": offsets, f"{name}_counts": counts, f"{name}_metrics": values, f"{name}_y_res": np.asarray(y_res)})
    print(f"case {name}: P={P} T={T} y_res={y_res} undecided={int((~decided).sum())} (lidar {int((~decided_lidar).sum())}) counts={counts.tolist()} "
          f"fp32-vs-fp64 table rel {rel:.1e} metrics={np.round(values, 4).tolist()}")
    return out


def generate():
    ev = load_evaluator()
    code = forward_statements(ev)
    ref = ref_shim.load_reference()
    from gen_golden import ref_conf, load_mlp_into
    cfg = O.FieldConfig()
    g = torch.Generator().manual_seed(NET["seed"])
    scene = O.synthetic_scene(1, NET["v"], NET["H"], NET["W"], NET["C"], seed=NET["seed"], smooth=True)
    mlp = O.init_mlp(NET["C"] + 39, NET["Hd"], 0, gen=g)
    mlp.b_out = torch.tensor([NET["b_out"]])
    net = ref.make_net(ref_conf(cfg, 0, NET["Hd"]), [scene["feat"]])
    load_mlp_into(net, mlp)
    net.eval()
    net.encode(scene["images"], scene["projs"], scene["poses"], ids_encoder=[0], ids_render=[1, 2])

    def sigma_of(q):
        with torch.no_grad():
            return net(q.unsqueeze(0), only_density=True)[2].reshape(-1)
    proj = scene["projs"][0, 0].contiguous()
    yy, xx = torch.meshgrid(torch.linspace(0, 1, NET["H"]), torch.linspace(0, 1, NET["W"]), indexing="ij")
    depth = (9 + 5 * torch.sin(5 * xx + 1) * torch.cos(3 * yy) + 3 * yy + 1.5 * torch.rand(NET["H"], NET["W"], generator=g)).contiguous()

    q_a = ev.get_pts(X_RANGE, Y_RANGE, Z_RANGE, 10, 4, 1)[0].reshape(-1, 3).contiguous()
    q_b = ev.get_pts(X_RANGE, Y_RANGE, Z_RANGE, 5, 4, 3)[0].reshape(-1, 3)[:-1].contiguous()
    assert q_a.shape[0] == 12800 and q_b.shape[0] % 3 == 2
    out = dict(proj=proj.numpy(), depth=depth.numpy(), net=np.array([NET[k] for k in ("seed", "H", "W", "C", "Hd", "v")]),
               net_b_out=np.asarray(NET["b_out"], dtype=np.float32), y_range=np.asarray(Y_RANGE, dtype=np.float64), max_dist=np.asarray(MAX_DIST),
               min_dist=np.asarray(MIN_DIST), occ_threshold=np.asarray(OCC_THRESHOLD))
    out.update(make_case(ev, code, "a", T=4, n_pts=3000, y_res=1, q_pts=q_a, seed=101, sigma_of=sigma_of, proj=proj, depth=depth,
                         empty=[{0, 1, 2, 120, 121, 122, 123}, {0, 1, 200, 201, 359}, {5, 6, 7, 300}, {0, 180, 181}]))
    out.update(make_case(ev, code, "b", T=3, n_pts=3000, y_res=3, q_pts=q_b, seed=202, sigma_of=sigma_of, proj=proj, depth=depth,
                         empty=[{0, 1, 2, 3, 77, 78}, {10, 11, 250, 251, 252}, {0, 358, 359}]))
    return out


if __name__ == "__main__":
    torch.set_num_threads(4)
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")
