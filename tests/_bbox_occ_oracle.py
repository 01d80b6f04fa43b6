"""A vectorised torch restatement of the 3D-bounding-box occupancy evaluation (the reference's models/bts/evaluator_3dbb.py: verts_to_cam,
bbox_in_frustum, compute_bounds, bbox_intercept_labeled with the argmin over boxes, in_bbox, project_into_cam, the two nearest look-ups
and the nine metrics), written from its behaviour.  dtype-generic (fp32 pins the kernels, fp64 gives the decision margins of the golden
fixture); runs on the CPU and, eagerly, on the GPU (tools/bbox_occ_probe.py times it there).

Boxes are lists: ``verts`` of (V, 3) world vertices, ``faces`` of (F, 3) integer tensors, ``labels`` of numbers."""
import torch
import torch.nn.functional as F

EPS = 1e-4
MARGIN = 1e-6            # a comparison is clear when it holds, or fails, by MARGIN * (1 + |p|)
DEPTH_REL, TIE_PX, SIGMA_ABS = 1e-5, 1e-3, 1e-3
METRIC_KEYS = ("o_acc", "o_rec", "o_prec", "no_nv_acc", "no_nv_rec", "no_nv_prec", "no_nv_r", "t_no_nv", "t_no_nop_nv")


def _inverse(m):
    """torch.inverse on the CPU (a tiny matrix; on a GPU it would pull in a solver library)"""
    return torch.inverse(m.cpu()).to(m.device)


def box_tables(verts, faces, pose, proj, max_d, eps_in=EPS):
    """-> fnbs: list of (F, 5) rows (nx, ny, nz, lo, hi) in the key frame; active: list of bools."""
    to_key = _inverse(pose)
    fnbs, active = [], []
    for v, f in zip(verts, faces):
        cam = (to_key[:3, :3] @ v.to(to_key.dtype).T + to_key[:3, 3, None]).T
        uv = (proj @ cam.T).T
        xy = uv[:, :2] / uv[:, 2:3]
        ok = (xy[:, 0] >= -1) & (xy[:, 0] <= 1) & (xy[:, 1] >= -1) & (xy[:, 1] <= 1) & (uv[:, 2] > 0) & (uv[:, 2] <= max_d)
        active.append(bool(ok.any()))
        f = f.long()
        n = torch.cross(cam[f[:, 1]] - cam[f[:, 0]], cam[f[:, 2]] - cam[f[:, 0]], dim=-1)
        n = n / torch.norm(n, dim=-1, keepdim=True)
        pr = n @ cam.T
        fnbs.append(torch.cat((n, pr.min(dim=-1, keepdim=True)[0], pr.max(dim=-1, keepdim=True)[0]), dim=-1))
    return fnbs, active


def padded_tables(fnbs, m_max=32):
    """the library's layout: (B, 32, 5) with zero rows past each box's faces, and the face counts"""
    out = torch.zeros((len(fnbs), m_max, 5), dtype=fnbs[0].dtype, device=fnbs[0].device)
    for b, t in enumerate(fnbs):
        out[b, :t.shape[0]] = t
    return out, torch.tensor([t.shape[0] for t in fnbs], dtype=torch.int32)


def resized_labels(seg, ph, pw):
    """F.interpolate(seg, (ph, pw), mode="nearest") -> (ph * pw)"""
    hs, ws = seg.shape[-2:]
    return F.interpolate(seg.reshape(1, 1, hs, ws), (ph, pw), mode="nearest").reshape(-1)


def _slabs(fnb, p, eps):
    """projections of the points p (N, 3) on the box's normals -> (m, N), and the widened bounds (m, 1)"""
    return fnb[:, :3] @ p.T, fnb[:, 3:4] - eps, fnb[:, 4:5] + eps


def in_bbox(p, fnb, eps=EPS):
    pr, lo, hi = _slabs(fnb, p, eps)
    return ((lo <= pr) & (pr <= hi)).all(dim=0)


def candidates(dirs, fnb):
    """(R, 2m, 3): p = (bound_j / (n_j . d)) d, the lower bounds first"""
    denom = fnb[:, :3] @ dirs.T
    i1 = (fnb[:, 3:4] / denom).T.unsqueeze(-1) * dirs.unsqueeze(1)
    i2 = (fnb[:, 4:5] / denom).T.unsqueeze(-1) * dirs.unsqueeze(1)
    return torch.cat((i1, i2), dim=1)


def pseudo_depth(dirs, ray_labels, fnbs, active, labels, eps=EPS, positive_z=True, use_labels=True):
    """-> (R): the smallest p_z over the valid candidates of the label-matching active boxes, +inf where there is none.
    eps / positive_z / use_labels exist for the fixture's mutants."""
    R = dirs.shape[0]
    best = torch.full((R,), float("inf"), dtype=dirs.dtype, device=dirs.device)
    for fnb, act, lab in zip(fnbs, active, labels):
        if not act:
            continue
        p = candidates(dirs, fnb)
        m2 = p.shape[1]
        flat = p.reshape(-1, 3)
        ok = in_bbox(flat, fnb, eps)
        if positive_z:
            ok = ok & (flat[:, 2] > 0)
        ok = ok.view(R, m2)
        if use_labels:
            ok = ok & (ray_labels.view(R, 1) == lab)
        z = torch.where(ok, p[:, :, 2], torch.full_like(p[:, :, 2], float("inf")))
        best = torch.minimum(best, z.min(dim=1)[0])
    return best


def decided_rays(dirs64, ray_labels, fnbs64, active, labels):
    """fp64 inputs.  A candidate is decided when every slab comparison and p_z > 0 hold by MARGIN * (1 + |p|), or at least one fails by
    it (a non-finite candidate fails); a ray when all candidates of its label-matching active boxes are."""
    R = dirs64.shape[0]
    decided = torch.ones(R, dtype=torch.bool, device=dirs64.device)
    for fnb, act, lab in zip(fnbs64, active, labels):
        if not act:
            continue
        p = candidates(dirs64, fnb)
        m2 = p.shape[1]
        flat = p.reshape(-1, 3)
        finite = torch.isfinite(flat).all(dim=-1)
        tol = MARGIN * (1 + torch.norm(flat, dim=-1))
        pr, lo, hi = _slabs(fnb, flat, EPS)
        holds = ((lo + tol <= pr) & (pr <= hi - tol)).all(dim=0) & (flat[:, 2] > tol)
        fails = ((pr < lo - tol) | (pr > hi + tol)).any(dim=0) | (flat[:, 2] < -tol) | ~finite | bool(torch.isnan(fnb).any())
        ok = (holds | fails).view(R, m2).all(dim=1)
        decided &= ok | (ray_labels != lab)
    return decided


def inside_any(q, fnbs, active):
    inside = torch.zeros(q.shape[0], dtype=torch.bool, device=q.device)
    for fnb, act in zip(fnbs, active):
        if act:
            inside |= in_bbox(q, fnb)
    return inside


def decided_inside(q64, fnbs64, active):
    decided = torch.ones(q64.shape[0], dtype=torch.bool, device=q64.device)
    tol = MARGIN * (1 + torch.norm(q64, dim=-1))
    for fnb, act in zip(fnbs64, active):
        if not act or bool(torch.isnan(fnb).any()):
            continue
        pr, lo, hi = _slabs(fnb, q64, EPS)
        holds = ((lo + tol <= pr) & (pr <= hi - tol)).all(dim=0)
        fails = ((pr < lo - tol) | (pr > hi + tol)).any(dim=0)
        decided &= holds | fails
    return decided


def lookups(q, proj, pseudo, depth_z):
    """project_into_cam and the two nearest, border-clamped, align_corners look-ups
    -> dist (P), gt (P), pred (P), pixel coordinates (P, 2) (x, y), the looked-up ray's index (P)."""
    cam = (proj @ q.T).T
    xy = cam[:, :2] / cam[:, 2:3]
    H, W = depth_z.shape
    grid = xy.view(1, 1, -1, 2)
    gt = F.grid_sample(pseudo.view(1, 1, H, W), grid, mode="nearest", padding_mode="border", align_corners=True).view(-1)
    pred = F.grid_sample(depth_z.view(1, 1, H, W), grid, mode="nearest", padding_mode="border", align_corners=True).view(-1)
    size = torch.tensor([W - 1, H - 1], dtype=q.dtype, device=q.device)
    pix = torch.minimum(torch.maximum((xy + 1) / 2 * size, torch.zeros_like(size)), size)
    idx = torch.round(pix[:, 1]).long() * W + torch.round(pix[:, 0]).long()
    return cam[:, 2], gt, pred, pix, idx


def masks(q, proj, pseudo, depth_z, fnbs, active, sigma, occ_threshold=0.5):
    """-> P, O, V (bool)"""
    dist, gt, pred, _, _ = lookups(q, proj, pseudo, depth_z)
    V = (dist <= gt) | (dist <= pred)
    O = inside_any(q, fnbs, active) & ~V
    return sigma > occ_threshold, O, V


def decided_points(q64, proj64, pseudo64, depth64, fnbs64, active, sigma, ray_decided, occ_threshold=0.5):
    dist, gt, pred, pix, idx = lookups(q64, proj64, pseudo64, depth64)
    frac = pix - torch.floor(pix)
    clear = ((dist - gt).abs() > DEPTH_REL * dist.abs()) & ((dist - pred).abs() > DEPTH_REL * dist.abs())
    return (decided_inside(q64, fnbs64, active) & clear & ((frac - 0.5).abs() > TIE_PX).all(dim=1) & ray_decided[idx]
            & ((sigma.double() - occ_threshold).abs() > SIGMA_ABS))


def cell_counts(P, O, V):
    """[V&P, V&!P, !V&O&P, !V&O&!P, !V&!O&P, !V&!O&!P]"""
    cells = [V & P, V & ~P, ~V & O & P, ~V & O & ~P, ~V & ~O & P, ~V & ~O & ~P]
    return [int(c.sum()) for c in cells]


def metrics(Pm, O, V):
    """The nine metrics as Python floats."""
    def mean(x):
        return x.float().mean().item()
    agree = (Pm == O)
    nonv = ~O & ~V
    return dict(o_acc=mean(agree), o_rec=mean(Pm[O]), o_prec=mean(O[Pm]), no_nv_acc=mean(agree[~V]), no_nv_rec=mean((~Pm)[nonv]),
                no_nv_prec=mean((~O)[~Pm & ~V]), no_nv_r=mean(nonv), t_no_nv=nonv.float().sum().item(),
                t_no_nop_nv=(~O & ~Pm)[nonv].float().sum().item())


def eager_frame(verts, faces, labels, pose, proj, max_d, dirs, seg, grid, depth_z, q, sigma, occ_threshold=0.5):
    """The reference's sequence per frame, box by box -> the six counts (what tools/bbox_occ_probe.py times on the GPU)."""
    fnbs, active = box_tables(verts, faces, pose, proj, max_d)
    pd = pseudo_depth(dirs, resized_labels(seg, *grid), fnbs, active, labels).view(*grid)
    return cell_counts(*masks(q, proj, pd, depth_z, fnbs, active, sigma, occ_threshold)), pd
