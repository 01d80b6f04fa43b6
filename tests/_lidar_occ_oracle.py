"""A vectorised torch restatement of the LiDAR occupancy evaluation (the reference's models/bts/evaluator_lidar.py: get_lidar_slices,
check_occupancy, project_into_cam, the nearest depth look-up and the nine metrics), written from its behaviour: a scatter_reduce(amin)
per (slice, cloud) instead of a Python loop over 360 bins, a cummax for the carry.  dtype-generic (fp32 pins the kernels, fp64 gives
the decision margins of the golden fixture); runs on the CPU and, eagerly, on the GPU (tools/occ_eval_probe.py times it there)."""
import math

import torch
import torch.nn.functional as F

N_BINS = 360


def _inverse(m):
    """torch.inverse on the CPU (tiny matrices; on a GPU it would pull in a solver library for 4 x 4 inverses)"""
    return torch.inverse(m.cpu()).to(m.device)


def slice_bounds(y_range, y_res, dtype=torch.float32, device="cpu"):
    """(lo, hi) of the y_res slices: the whole range for one slice, else the linspace levels +- half their spacing."""
    ys = torch.linspace(y_range[0], y_range[1], y_res, dtype=dtype, device=device)
    if y_res == 1:
        return ys.clone(), torch.full_like(ys, y_range[-1])
    half = (ys[1] - ys[0]) / 2
    return ys - half, ys + half


def lidar_tables(point_clouds, velo_poses, y_range, y_res, max_dist):
    """-> (y_res, T, 362, 2): (angle, distance) rows per (slice, cloud), wrap rows included."""
    dtype, dev = point_clouds[0].dtype, point_clouds[0].device
    borders = torch.linspace(-math.pi, math.pi, N_BINS + 1, dtype=dtype).to(dev)
    centres = (borders[:-1] + borders[1:]) * .5
    lo, hi = slice_bounds(y_range, y_res, dtype, dev)
    inf = torch.tensor(float("inf"), dtype=dtype, device=dev)
    out = torch.empty((y_res, len(point_clouds), N_BINS + 2, 2), dtype=dtype, device=dev)
    for t, (pc, pose) in enumerate(zip(point_clouds, velo_poses)):
        world = (pose @ pc.T).T
        far = torch.norm(world[:, :3], dim=-1) >= max_dist
        xy = pc[:, :2].contiguous()
        angles, dists = torch.atan2(xy[:, 1], xy[:, 0]), torch.norm(xy, dim=-1)
        bins = torch.searchsorted(borders, angles.contiguous(), right=True) - 1      # bin i = [border_i, border_i+1)
        in_bin = (bins >= 0) & (bins < N_BINS)
        for s in range(y_res):
            sel = ((world[:, 1] >= lo[s]) & (world[:, 1] <= hi[s])) | far
            use = sel & in_bin
            mins = torch.full((N_BINS,), float("inf"), dtype=dtype, device=dev).scatter_reduce(0, bins[use], dists[use], "amin")
            first = dists[sel][torch.argmin(angles[sel])] if bool(sel.any()) else inf   # the carry's initial value
            filled = torch.where(torch.isinf(mins), torch.full((N_BINS,), -1, dtype=torch.long, device=dev), torch.arange(N_BINS, device=dev))
            src = torch.cummax(filled, dim=0)[0]
            d = torch.where(src >= 0, mins[src.clamp_min(0)], first)
            out[s, t, 1:-1, 0], out[s, t, 1:-1, 1] = centres, d
            out[s, t, 0, 0], out[s, t, 0, 1] = centres[-1] - math.pi * 2, d[-1]
            out[s, t, -1, 0], out[s, t, -1, 1] = centres[0] + math.pi * 2, d[0]
    return out


def occupancy_terms(pts, tables, velo_poses):
    """Per slice i (which owns pts[i * step : (i + 1) * step]): dists (T, step), surface (T, step) -- the two sides of the per-cloud test."""
    y_res, T = tables.shape[:2]
    step = pts.shape[0] // y_res
    hom = torch.cat((pts, torch.ones_like(pts[:, :1])), dim=-1)
    world_to_velo = _inverse(velo_poses)
    terms = []
    for i in range(y_res):
        chunk = hom[i * step:(i + 1) * step]
        dists, surface = [], []
        for j in range(T):
            velo = (world_to_velo[j] @ chunk.T).T
            angles = torch.atan2(velo[:, 1], velo[:, 0])
            tab_a, tab_d = tables[i, j, :, 0].contiguous(), tables[i, j, :, 1].contiguous()
            right = torch.searchsorted(tab_a, angles)
            w = (angles - tab_a[right - 1]) / (tab_a[right] - tab_a[right - 1])
            surface.append(tab_d[right - 1] * (1 - w) + tab_d[right] * w)
            dists.append(torch.norm(velo, dim=-1))        # all four components, as the reference
        terms.append((torch.stack(dists), torch.stack(surface)))
    return terms


def check_occupancy(pts, tables, velo_poses, min_dist=3):
    """-> is_occupied (P) bool, is_visible (P) bool."""
    y_res, T = tables.shape[:2]
    step = pts.shape[0] // y_res
    votes = torch.ones_like(pts[:, 0])
    visible = torch.zeros_like(pts[:, 0], dtype=torch.bool)
    for i, (dists, surface) in enumerate(occupancy_terms(pts, tables, velo_poses)):
        occ = (dists > surface) | (dists < min_dist)
        votes[i * step:(i + 1) * step] += occ.to(votes.dtype).sum(dim=0)
        visible[i * step:(i + 1) * step] = ~occ[0]
    votes /= T
    return votes > (T - 2) / T, visible


def predicted_visibility(pts, proj, pose, depth_z):
    """project_into_cam + the nearest, border-clamped, align_corners look-up: -> dist (P), pred_dist (P), pixel coordinates (P, 2)."""
    hom = torch.cat((pts, torch.ones_like(pts[:, :1])), dim=-1)
    cam = (proj @ (_inverse(pose)[:3, :] @ hom.T)).T
    xy = cam[:, :2] / cam[:, 2:3]
    H, W = depth_z.shape
    pred = F.grid_sample(depth_z.view(1, 1, H, W), xy.view(1, 1, -1, 2), mode="nearest", padding_mode="border", align_corners=True).view(-1)
    size = torch.tensor([W - 1, H - 1], dtype=pts.dtype, device=pts.device)
    pix = torch.minimum(torch.maximum((xy + 1) / 2 * size, torch.zeros_like(size)), size)
    return cam[:, 2], pred, pix


def cell_counts(P, O, V):
    """[V&P, V&!P, !V&O&P, !V&O&!P, !V&!O&P, !V&!O&!P]"""
    cells = [V & P, V & ~P, ~V & O & P, ~V & O & ~P, ~V & ~O & P, ~V & ~O & ~P]
    return [int(c.sum()) for c in cells]


def metrics(is_occupied, is_visible, is_visible_pred, is_occupied_pred):
    """The nine metrics; V = is_visible | is_visible_pred, O = is_occupied & ~V.  -> dict of Python floats, and (P, O, V)."""
    V = is_visible | is_visible_pred
    O = is_occupied & ~V
    Pm = is_occupied_pred
    agree = (Pm == O).float()
    ie = ~O & ~V

    def mean(x):
        return x.float().mean().item()
    out = dict(o_acc=mean(agree), o_prec=mean(O[Pm]), o_rec=mean(Pm[O]), ie_r=mean(ie), t_ie=ie.float().sum().item(), ie_acc=mean(agree[~V]),
               ie_prec=mean((~O)[~Pm & ~V]), ie_rec=mean((~Pm)[ie]), t_no_nop_nv=(~O & ~Pm)[ie].float().sum().item())
    return out, (Pm, O, V)
