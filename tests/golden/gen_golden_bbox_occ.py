"""Golden fixture for the 3D-bounding-box occupancy evaluation FROM THE REAL REFERENCE.  Run in the build container only:

    python -B tests/golden/gen_golden_bbox_occ.py

Imports the reference's models/bts/evaluator_3dbb.py unmodified (its third-party imports -- ignite, the dataset factory, the evaluation
driver, the metric class -- are stubbed here before the import; oracle/ref_shim.py supplies the rest) and runs its verts_to_cam,
bbox_in_frustum, compute_bounds, bbox_intercept_labeled, in_bbox, get_pts, project_into_cam and the statements of BTSWrapper.forward
that form the pseudo depth, the two look-ups, the occupancy and the nine metrics (cut out of the source as AST nodes and executed
unmodified) on the CPU, in fp32 and, for arbitration, in fp64 on the same fp32 inputs.  Nothing of the reference's source enters the
repository; the inputs and outputs do: tests/golden/bbox_occ.npz.

Case A: a 48 x 160 frame, 24 x 80 rays, the label map at 48 x 160, the evaluator's 13 600 query points, 14 boxes: seven yawed cuboids
(one in front of another with a different label), one behind the camera, one outside the frustum, one beyond max_d, one around the
camera (it straddles z = 0), one `flat` slab (id 7), one pentagonal prism (10 vertices, 16 faces), one cuboid with a degenerate face.
About 20 % of the pixels carry a label no box has.  Case B: 23 x 77 rays under a 47 x 155 label map, one active box, P = 999.

The generator stores a per-ray and a per-point `decided` mask (tests/_bbox_occ_oracle.py: decided_rays, decided_points; fp64 on the
fp32 inputs) and ASSERTS, on the reference alone: at most 1 % of the rays and of the points undecided; fp32 and fp64 agree on every
decided element; all six cells non-empty in case A; at least three boxes inactive; the occluded box changes the pseudo depth of at
least one ray; the mutants EPS = 0, no p_z > 0, no labels, max_d = 80 land outside the bars on decided elements.  pd_ref_rel is the
fp32 reference's largest relative distance to its own fp64 run over decided finite rays; the GPU tests' bar is 4 x that."""
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
import _bbox_occ_oracle as BO

OUT = os.path.join(HERE, "bbox_occ.npz")
X_RANGE, Y_RANGE, Z_RANGE, PPM, PPM_Y = (-4, 4), (0, 1), (20, 3), 5, 4
MAX_D, OCC_THRESHOLD, Z_NEAR, Z_FAR = Z_RANGE[0], 0.5, 3.0, 80.0
FLAT_IDS = (7, 8, 9, 10)
NET = dict(seed=5, H=48, W=160, C=64, Hd=64, v=3, b_out=1.2)   # the encoded net of lidar_occ.npz, rebuilt from its seed
NO_BOX_LABELS = (0.0, 11.0, 23.0)                               # labels no box carries
METRIC_NAMES = dict(o_acc="is_occupied_acc", o_rec="is_occupied_rec", o_prec="is_occupied_prec", no_nv_acc="no_nv_acc", no_nv_rec="no_nv_rec",
                    no_nv_prec="no_nv_prec", no_nv_r="not_occupied_not_visible_ratio", t_no_nv="total_no_nv", t_no_nop_nv="total_no_nop_nv")


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
    import models.bts.evaluator_3dbb as ev
    flat = tuple(sorted(i for i, l in ev.id2label.items() if l.category == "flat"))
    assert flat == FLAT_IDS, flat
    return ev


def forward_statements(ev):
    """Code objects cut out of BTSWrapper.forward, unmodified: the pseudo depth (`bbox_intercept_labeled_ = ...` to `pseudo_depth = ...`),
    the look-ups (`cam_pts, dists = ...` to `is_visible = ...`), the occupancy (`is_occupied = ...` to `is_occupied &= ~is_visible`) and
    the metrics (`is_occupied_acc = ...` to `total_no_nop_nv = ...`)."""
    path = ev.__file__
    tree = ast.parse(open(path).read())
    body = next(f for c in tree.body if isinstance(c, ast.ClassDef) and c.name == "BTSWrapper"
                for f in c.body if isinstance(f, ast.FunctionDef) and f.name == "forward").body

    def first_name(s):
        if isinstance(s, ast.Assign):
            t = s.targets[0]
            return t.elts[0].id if isinstance(t, ast.Tuple) else getattr(t, "id", "")
        if isinstance(s, ast.AugAssign):
            return "aug:" + getattr(s.target, "id", "")
        return ""

    def at(name):
        return next(i for i, s in enumerate(body) if first_name(s) == name)

    def cut(a, b):
        return compile(ast.Module(body=body[at(a):at(b) + 1], type_ignores=[]), path, "exec")
    return dict(pseudo=cut("bbox_intercept_labeled_", "pseudo_depth"), lookup=cut("cam_pts", "is_visible"), occupied=cut("is_occupied", "aug:is_occupied"),
                metrics=cut("is_occupied_acc", "total_no_nop_nv"))


class _Torch64:
    """torch with float32 spelled float64: verts_to_cam casts the vertices to torch.float32 by name (:31); the fp64 run keeps them fp64"""

    def __getattr__(self, k):
        return torch.float64 if k == "float32" else getattr(torch, k)


# ---- scene ------------------------------------------------------------------------------------------------------------------------
QUADS = ((0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5))


def _yaw(pts, centre, yaw_deg):
    a = math.radians(yaw_deg)
    c, s = math.cos(a), math.sin(a)
    x, z = pts[:, 0].clone(), pts[:, 2].clone()
    pts[:, 0], pts[:, 2] = c * x + s * z, -s * x + c * z
    return pts + torch.tensor(centre, dtype=torch.float64)


def cuboid(centre, size, yaw_deg):
    """8 vertices / 12 triangles in the key frame (y down), yawed about the vertical"""
    half = torch.tensor(size, dtype=torch.float64) / 2
    corners = torch.tensor([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=torch.float64) * half
    faces = torch.tensor([t for a, b, c, d in QUADS for t in ((a, b, c), (a, c, d))], dtype=torch.int64)
    return _yaw(corners, centre, yaw_deg), faces


def prism(centre, radius, height, yaw_deg):
    """a pentagonal prism: 10 vertices / 16 triangles"""
    ring = [[radius * math.cos(2 * math.pi * k / 5), y, radius * math.sin(2 * math.pi * k / 5)] for y in (-height / 2, height / 2) for k in range(5)]
    faces = [t for k in range(5) for t in ((k, (k + 1) % 5, (k + 1) % 5 + 5), (k, (k + 1) % 5 + 5, k + 5))]
    faces += [(0, 1, 2), (0, 2, 3), (0, 3, 4), (5, 6, 7), (5, 7, 8), (5, 8, 9)]
    return _yaw(torch.tensor(ring, dtype=torch.float64), centre, yaw_deg), torch.tensor(faces, dtype=torch.int64)


def grid_y(z):
    """the height of the middle of the query grid at depth z"""
    return 0.5 - 0.0874886635 * z


def scene_a():
    """(name, key-frame vertices fp64, faces, semantic id)"""
    def car(x, z, yaw, label, size=(1.9, 1.7, 4.2)):
        return cuboid((x, grid_y(z), z), size, yaw) + (label,)
    boxes = [("front", *car(-1.4, 6.5, 12, 26.0)), ("occluded", *car(-1.9, 11.5, -8, 27.0, (3.2, 2.4, 5.0))),
             ("c2", *car(1.9, 5.2, -20, 26.0)), ("c3", *car(2.6, 10.0, 25, 28.0)), ("c4", *car(0.3, 13.5, 80, 26.0)),
             ("c5", *car(-3.2, 16.5, 5, 24.0, (1.0, 1.9, 1.0))), ("c6", *car(3.3, 17.0, -35, 27.0)),
             ("behind", *car(0.5, -6.0, 10, 26.0)), ("outside", *car(40.0, 5.0, 0, 26.0)), ("far", *cuboid((-0.5, -8.0, 26.0), (3.0, 2.5, 5.0), 15), 28.0),
             ("around", *cuboid((0.1, 0.1, 1.05), (1.2, 1.0, 5.1), 3), 34.0), ("flat", *cuboid((0.0, 1.2, 11.5), (8.0, 0.3, 17.0), 0), 7.0),
             ("prism", *prism((-0.2, grid_y(8.5), 8.5), 1.1, 1.8, 17), 33.0), ("degenerate", *car(0.9, 16.8, 40, 26.0))]
    name, v, f, lab = boxes[-1]
    f = f.clone()
    f[4] = torch.tensor([f[4, 0], f[4, 0], f[4, 2]])          # two equal vertices: a zero cross product, a NaN normal
    boxes[-1] = (name, v, f, lab)
    return boxes


def scene_b():
    return [("only", *cuboid((0.4, grid_y(8.0), 8.0), (3.0, 2.2, 4.5), 22), 26.0), ("behind", *cuboid((0.0, 0.0, -5.0), (2.0, 2.0, 4.0), 0), 27.0)]


def to_world(v_key, pose):
    p = pose.double()
    return (p[:3, :3] @ v_key.T + p[:3, 3, None]).T.float().contiguous()


def key_rays(ref, pose, proj, h, w):
    """the rays of the reference's own sampler in the key frame (:229-231): (h * w, 8) fp32"""
    sampler = ref.ImageRaySampler(Z_NEAR, Z_FAR, channels=1)
    sampler.height, sampler.width = h, w
    poses = (torch.inverse(pose) @ pose).view(1, 1, 4, 4)
    rays, _ = sampler.sample(None, poses, proj.view(1, 1, 3, 3))
    return rays[0].contiguous()


def paint_labels(ref, boxes, pose, proj, hs, ws, gen, patch):
    """The label map: the label of the nearest box along the pixel's ray, a random box's label where there is none (the box around the camera and the flat slab left out; the
    degenerate box painted from its clean geometry), 12 % of the pixels re-labelled at random among the boxes' labels, 20 % with a
    label no box has, and a patch of the label of the box around the camera."""
    dirs = key_rays(ref, pose, proj, hs, ws)[:, 3:6].double()
    labs = torch.tensor(sorted({lab for _, _, _, lab in boxes if lab not in FLAT_IDS}), dtype=torch.float64)
    seg = labs[torch.randint(len(labs), (hs * ws,), generator=gen)]          # where no box is: some box's label all the same
    best = torch.full((hs * ws,), float("inf"), dtype=torch.float64)
    for name, v, f, lab in boxes:
        if name in ("around", "flat"):
            continue
        if name == "degenerate":
            f = cuboid((0, 0, 0), (1, 1, 1), 0)[1]
        fnbs, act = BO.box_tables([to_world(v, pose).double()], [f], pose.double(), proj.double(), MAX_D)
        z = BO.pseudo_depth(dirs, seg, fnbs, [True], [lab], use_labels=False)
        seg = torch.where(z < best, torch.full_like(seg, lab), seg)
        best = torch.minimum(best, z)
    u = torch.rand(hs * ws, generator=gen)
    seg = torch.where(u < 0.12, labs[torch.randint(len(labs), (hs * ws,), generator=gen)], seg)
    none = torch.tensor(NO_BOX_LABELS, dtype=torch.float64)
    seg = torch.where(u > 0.80, none[torch.randint(len(none), (hs * ws,), generator=gen)], seg)
    seg = seg.view(hs, ws)
    if patch is not None:
        (y0, y1, x0, x1), lab = patch
        seg[y0:y1, x0:x1] = lab
    return seg.float().contiguous()


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def reference_run(ev, ref, code, raw, seg, rays, grid, pose, proj, depth, q_pts, sigma, dtype):
    """BTSWrapper.forward without the render, in `dtype`.  raw: list of (world vertices fp32, faces, id)."""
    ph, pw = grid
    real_torch = ev.torch
    torch.set_default_dtype(dtype)
    if dtype == torch.float64:
        ev.torch = _Torch64()
    try:
        pose, proj, depth, q_pts, seg, rays = (t.to(dtype) for t in (pose, proj, depth, q_pts, seg, rays))
        bboxes = [dict(vertices=v[None].to(dtype), faces=f[None].clone(), semanticId=torch.tensor(int(lab))) for v, f, lab in raw]
        bboxes = [b for b in bboxes if ev.id2label[b["semanticId"].item()].category != "flat"]                      # :201
        to_keyframe = torch.inverse(pose.view(1, 1, 4, 4))                                                          # :212
        bboxes = [ev.verts_to_cam(b, to_keyframe[0, 0]) for b in bboxes]                                            # :218
        active = [bool(ev.bbox_in_frustum(b, proj, MAX_D, reducer=torch.any)) for b in bboxes]                      # :219
        all_fnbs = [ev.compute_bounds(b) for b in bboxes]          # (the library forms every box's table; the reference the active ones')
        kept = [b for b, a in zip(bboxes, active) if a]
        fnbs = [t for t, a in zip(all_fnbs, active) if a]                                                           # :226
        labels = torch.tensor([b["semanticId"] for b in kept])                                                      # :227
        gt_label = F.interpolate(seg.view(1, 1, *seg.shape), (ph, pw), mode="nearest").permute(0, 2, 3, 1).reshape(1, -1, 1)   # :231, 250-251
        ns = dict(ev.__dict__, torch=torch, F=F, dirs=rays[:, 3:6].reshape(-1, 3), gt_label=gt_label, fnbs=fnbs, labels=labels, ph=ph, pw=pw)
        exec(code["pseudo"], ns)
        pseudo_depth = ns["pseudo_depth"]
        ns.update(q_pts=q_pts, projs=proj.view(1, 1, 3, 3), pred_depth=depth, bboxes=kept, is_occupied_pred=sigma > OCC_THRESHOLD)
        exec(code["lookup"], ns)
        exec(code["occupied"], ns)
        exec(code["metrics"], ns)
        values = np.array([float(ns[METRIC_NAMES[k]]) for k in BO.METRIC_KEYS], dtype=np.float64)
        return dict(all_fnbs=all_fnbs, active=active, pseudo=pseudo_depth.reshape(-1).clone(), P=ns["is_occupied_pred"], O=ns["is_occupied"],
                    V=ns["is_visible"], metrics=values, dists=ns["dists"], gt_dist=ns["gt_dist"], pred_dist=ns["pred_dist"])
    finally:
        ev.torch = real_torch
        torch.set_default_dtype(torch.float32)


def make_case(ev, ref, code, name, *, boxes, grid, seg_size, q_pts, sigma_of, pose, proj, gen, patch, full):
    ph, pw = grid
    raw = [(to_world(v, pose), f, lab) for _, v, f, lab in boxes]
    names = [n for n, _, _, lab in boxes if lab not in FLAT_IDS]
    seg = paint_labels(ref, boxes, pose, proj, *seg_size, gen, patch)
    rays = key_rays(ref, pose, proj, ph, pw)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, ph), torch.linspace(0, 1, pw), indexing="ij")
    depth = (5 + 3 * torch.sin(5 * xx + 1) * torch.cos(3 * yy) + 2 * yy + torch.rand(ph, pw, generator=gen)).contiguous()
    sigma = sigma_of(q_pts)
    P, R = q_pts.shape[0], ph * pw

    r32 = reference_run(ev, ref, code, raw, seg, rays, grid, pose, proj, depth, q_pts, sigma, torch.float32)
    r64 = reference_run(ev, ref, code, raw, seg, rays, grid, pose, proj, depth, q_pts, sigma, torch.float64)
    active = r32["active"]
    assert active == r64["active"], (active, r64["active"])
    kept = [(v, f, lab) for v, f, lab in raw if lab not in FLAT_IDS]
    verts, faces, labels = [v for v, _, _ in kept], [f for _, f, _ in kept], [lab for _, _, lab in kept]
    B = len(kept)

    # ---- the restatement is the reference (fp32: what the CPU test repeats; fp64: what the decided masks stand on)
    fnbs64, act64 = BO.box_tables([v.double() for v in verts], faces, pose.double(), proj.double(), MAX_D)
    assert act64 == active
    for a, b in zip(fnbs64, r64["all_fnbs"]):
        assert torch.allclose(a, b, rtol=0, atol=1e-12, equal_nan=True)
    ray_labels = BO.resized_labels(seg, ph, pw)
    dirs64 = rays[:, 3:6].double()
    pd64 = BO.pseudo_depth(dirs64, ray_labels.double(), fnbs64, active, labels)
    assert torch.equal(torch.isfinite(pd64), torch.isfinite(r64["pseudo"]))
    fin64 = torch.isfinite(pd64)
    assert torch.allclose(pd64[fin64], r64["pseudo"][fin64], rtol=1e-12, atol=0)

    # ---- decided rays, the reference's own error
    decided_ray = BO.decided_rays(dirs64, ray_labels.double(), fnbs64, active, labels)
    assert int((~decided_ray).sum()) <= R // 100, (name, int((~decided_ray).sum()), R)
    assert torch.equal(torch.isfinite(r32["pseudo"])[decided_ray], fin64[decided_ray])
    sel = decided_ray & fin64
    pd_ref_rel = ((r32["pseudo"].double() - r64["pseudo"]).abs() / r64["pseudo"])[sel].max().item()
    tab32, n_faces = BO.padded_tables(r32["all_fnbs"])
    tab64, _ = BO.padded_tables(r64["all_fnbs"])
    assert torch.equal(torch.isnan(tab32), torch.isnan(tab64))
    diff = torch.nan_to_num((tab32.double() - tab64).abs(), nan=0.0)
    normal_ref_abs, bound_ref_abs = diff[..., :3].max().item(), diff[..., 3:].max().item()

    # ---- decided points
    decided_pt = BO.decided_points(q_pts.double(), proj.double(), r64["pseudo"].view(ph, pw), depth.double(), fnbs64, active, sigma, decided_ray)
    assert int((~decided_pt).sum()) <= P // 100, (name, int((~decided_pt).sum()), P)
    for k in ("P", "O", "V"):
        assert torch.equal(r32[k][decided_pt], r64[k][decided_pt]), k
    counts = BO.cell_counts(r32["P"], r32["O"], r32["V"]) + [sum(active)]
    assert sum(counts[:6]) == P

    # ---- the scene's own conditions
    pd_bar = 4 * pd_ref_rel
    if full:
        assert all(c > 0 for c in counts[:6]), counts
        assert B - sum(active) >= 3, active
        assert not active[names.index("behind")] and not active[names.index("outside")] and not active[names.index("far")]
        assert active[names.index("around")] and active[names.index("degenerate")] and active[names.index("occluded")]
        assert torch.isnan(tab32[names.index("degenerate")]).any()
        without = [a and n != "occluded" for a, n in zip(active, names)]
        assert (BO.pseudo_depth(dirs64, ray_labels.double(), fnbs64, without, labels) != pd64).any()
        frac_none = float(sum((seg == l).float().mean() for l in NO_BOX_LABELS))
        assert 0.15 < frac_none < 0.3, frac_none

        def outside_bar(pd):
            fin = torch.isfinite(pd)
            bad = fin != fin64
            both = fin & fin64
            bad[both] |= ((pd[both] - pd64[both]).abs() / pd64[both].abs()) > pd_bar
            return int((bad & decided_ray).sum())
        mutants = dict(eps0=outside_bar(BO.pseudo_depth(dirs64, ray_labels.double(), fnbs64, active, labels, eps=0.0)),
                       no_pz=outside_bar(BO.pseudo_depth(dirs64, ray_labels.double(), fnbs64, active, labels, positive_z=False)),
                       no_labels=outside_bar(BO.pseudo_depth(dirs64, ray_labels.double(), fnbs64, active, labels, use_labels=False)))
        _, act80 = BO.box_tables([v.double() for v in verts], faces, pose.double(), proj.double(), 80)
        mutants["max_d_80"] = outside_bar(BO.pseudo_depth(dirs64, ray_labels.double(), fnbs64, act80, labels))
        assert all(v > 0 for v in mutants.values()), mutants
        print("mutants (decided rays outside the bar):", mutants)
    else:
        assert sum(active) == 1

    v_off = np.cumsum([0] + [v.shape[0] for v, _, _ in raw]).astype(np.int32)
    f_off = np.cumsum([0] + [f.shape[0] for _, f, _ in raw]).astype(np.int32)
    arrays = dict(raw_vertices=torch.cat([v for v, _, _ in raw]), raw_faces=torch.cat([f for _, f, _ in raw]).to(torch.int32),
                  raw_semantic_id=torch.tensor([lab for _, _, lab in raw], dtype=torch.float32), seg=seg, rays=rays, depth=depth, q_pts=q_pts,
                  sigma=sigma, pose=pose, tables=tab32, n_faces=n_faces, active=torch.tensor(active), pseudo=r32["pseudo"].view(ph, pw),
                  pseudo64=r64["pseudo"].view(ph, pw), decided_ray=decided_ray, decided=decided_pt, mask_P=r32["P"], mask_O=r32["O"], mask_V=r32["V"])
    out = {f"{name}_{k}": v.numpy() for k, v in arrays.items()}
    out.update({f"{name}_raw_v_offsets": v_off, f"{name}_raw_f_offsets": f_off, f"{name}_counts": np.array(counts, dtype=np.int32),
                f"{name}_metrics": r32["metrics"], f"{name}_grid": np.array(grid, dtype=np.int32), f"{name}_pd_ref_rel": np.asarray(pd_ref_rel),
                f"{name}_pd_bar": np.asarray(pd_bar), f"{name}_normal_ref_abs": np.asarray(normal_ref_abs),
                f"{name}_bound_ref_abs": np.asarray(bound_ref_abs)})
    print(f"case {name}: R={R} P={P} B={B} active={sum(active)} finite rays={int(fin64.sum())} undecided rays={int((~decided_ray).sum())} "
          f"undecided points={int((~decided_pt).sum())} counts={counts} pd_ref_rel={pd_ref_rel:.2e} (bar {pd_bar:.2e}) "
          f"table fp32-vs-fp64 normal {normal_ref_abs:.1e} bound {bound_ref_abs:.1e} metrics={np.round(r32['metrics'], 4).tolist()}")
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
    pose = O._pose(tx=0.05, ty=-0.03, tz=0.1, yaw_deg=2.0)

    grid_pts, dims = ev.get_pts(X_RANGE, Y_RANGE, Z_RANGE, PPM, PPM_Y)
    q_a = grid_pts.reshape(-1, 3).contiguous()
    assert q_a.shape[0] == 13600 and dims == (40, 4, 85)
    q_b = q_a[::13][:999].contiguous()
    assert q_b.shape[0] == 999
    out = dict(proj=proj.numpy(), net=np.array([NET[k] for k in ("seed", "H", "W", "C", "Hd", "v")]),
               net_b_out=np.asarray(NET["b_out"], dtype=np.float32), max_d=np.asarray(MAX_D), occ_threshold=np.asarray(OCC_THRESHOLD),
               flat_ids=np.array(FLAT_IDS, dtype=np.int32))
    out.update(make_case(ev, ref, code, "a", boxes=scene_a(), grid=(24, 80), seg_size=(48, 160), q_pts=q_a, sigma_of=sigma_of, pose=pose, proj=proj,
                         gen=torch.Generator().manual_seed(303), patch=((30, 40, 66, 86), 34.0), full=True))
    out.update(make_case(ev, ref, code, "b", boxes=scene_b(), grid=(23, 77), seg_size=(47, 155), q_pts=q_b, sigma_of=sigma_of, pose=pose, proj=proj,
                         gen=torch.Generator().manual_seed(404), patch=None, full=False))
    return out


if __name__ == "__main__":
    torch.set_num_threads(4)
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")
