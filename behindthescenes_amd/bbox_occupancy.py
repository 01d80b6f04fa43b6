"""The 3D-bounding-box occupancy evaluation of the reference (models/bts/evaluator_3dbb.py) on the HIP kernels of csrc/bts_bbox_occ.hip.

``get_pts`` keeps the reference's signature; ``pack_bboxes`` turns the data loader's list of box dicts into the packed tensors the
library reads; ``bbox_tables`` and ``pseudo_depth`` are the two ground-truth stages on their own.  ``FusedBBoxOccupancyEval`` runs the
whole frame after the render -- box bounds, pseudo depth, density query, visibility, occupancy and the counts behind the nine metrics --
from ONE library call (bts_bbox_occupancy_eval) and one device-to-host copy of seven integers.
There is no torch fallback: CPU tensors are rejected, as everywhere else in this package."""
import ctypes as C

import torch

from . import _lib, native
from ._evalcommon import FusedOccupancy, occupancy_ratios, proj3 as _proj3
from ._lib import BtsNativeError
from .native import _addr, _ptr, _req, _req_as, _stream

M_MAX = _lib.BTS_BBOX_MAX_FACES
# the ids KITTI-360's label table puts in category `flat`: road, sidewalk, parking, rail track (evaluator_3dbb.py:201)
FLAT_SEMANTIC_IDS = (7, 8, 9, 10)
METRIC_KEYS = ("o_acc", "o_rec", "o_prec", "no_nv_acc", "no_nv_rec", "no_nv_prec", "no_nv_r", "t_no_nv", "t_no_nop_nv")


def get_pts(x_range, y_range, z_range, ppm, ppm_y):
    """The evaluator's query grid (evaluator_3dbb.py:131-143): (y_res, z_res, x_res, 3) key-frame points on the CPU, x fastest, lowered by
    z * tan(5 degrees) for the cameras' inclination, and the three sizes."""
    x_res = abs(int((x_range[1] - x_range[0]) * ppm))
    y_res = abs(int((y_range[1] - y_range[0]) * ppm_y))
    z_res = abs(int((z_range[1] - z_range[0]) * ppm))
    xs, ys, zs = (torch.linspace(r[0], r[1], n) for r, n in ((x_range, x_res), (y_range, y_res), (z_range, z_res)))
    grid = torch.empty((y_res, z_res, x_res, 3))
    grid[..., 0], grid[..., 1], grid[..., 2] = xs.view(1, 1, -1), ys.view(-1, 1, 1), zs.view(1, -1, 1)
    grid[..., 1] -= grid[..., 2] * 0.0874886635
    return grid, (x_res, y_res, z_res)


def pack_bboxes(bboxes, skip_semantic_ids=FLAT_SEMANTIC_IDS):
    """The data loader's list of dicts (``vertices`` (1, V, 3), ``faces`` (1, F, 3), ``semanticId``) without the `flat` boxes
    -> vertices (sum V, 3) fp32, faces (sum F, 3) int32, semantic_id (B) fp32 on the boxes' device, and the two HOST offset arrays
    (ctypes int32, B + 1 entries each).  The ids are read on the host, as the reference's `.item()` at :201 reads them: keep them CPU
    tensors or numbers, or pack once per frame and hand the tuple to FusedBBoxOccupancyEval."""
    skip = set(int(i) for i in skip_semantic_ids)
    kept = [b for b in bboxes if int(b["semanticId"]) not in skip]
    n = len(kept)
    v_off, f_off = (C.c_int32 * (n + 1))(), (C.c_int32 * (n + 1))()
    verts, faces = [], []
    for k, b in enumerate(kept):
        v, f = b["vertices"], b["faces"]
        v, f = v.reshape(-1, 3).to(torch.float32), f.reshape(-1, 3).to(torch.int32)
        verts.append(v), faces.append(f)
        v_off[k + 1], f_off[k + 1] = v_off[k] + v.shape[0], f_off[k] + f.shape[0]
    dev = verts[0].device if n else torch.device("cpu")
    vertices = torch.cat(verts, dim=0).contiguous() if n else torch.zeros((0, 3), dtype=torch.float32)
    faces = torch.cat(faces, dim=0).contiguous() if n else torch.zeros((0, 3), dtype=torch.int32)
    semantic_id = torch.tensor([float(b["semanticId"]) for b in kept], dtype=torch.float32).to(dev)
    return vertices, faces, semantic_id, v_off, f_off


def _req_boxes(vertices, faces, semantic_id, v_off, f_off, what):
    B = len(v_off) - 1
    if B <= 0 or len(f_off) != B + 1:
        raise BtsNativeError(f"{what}: no boxes (none given, or every box is of a skipped category)")
    _req(vertices, "vertices", (v_off[B], 3))
    _req_as(faces, "faces", torch.int32, (f_off[B], 3))
    if semantic_id is not None:
        _req(semantic_id, "semantic_id", (B,))
    return B


def bbox_tables(vertices, faces, v_offsets, f_offsets, pose, proj, max_d=20):
    """verts_to_cam, bbox_in_frustum and compute_bounds (evaluator_3dbb.py:30-60) for all boxes at once  (bts_bbox_bounds).
    ``pose`` (4, 4) is the encoder view's camera-to-world pose (poses[0, 0]), ``proj`` its normalised intrinsics.
    -> tables (B, 32, 5) rows of (nx, ny, nz, lo, hi), n_faces (B) int32, active (B) uint8."""
    B = _req_boxes(vertices, faces, None, v_offsets, f_offsets, "bbox_tables")
    dev = vertices.device
    to_key = native.invert_small(_req(pose.reshape(4, 4) if isinstance(pose, torch.Tensor) else pose, "pose", (4, 4)))   # torch.inverse at :212
    tables = torch.empty((B, M_MAX, 5), device=dev, dtype=torch.float32)
    n_faces = torch.empty(B, device=dev, dtype=torch.int32)
    active = torch.empty(B, device=dev, dtype=torch.uint8)
    _lib.check(_lib.load().bts_bbox_bounds(_ptr(vertices), _ptr(faces), v_offsets, f_offsets, B, _ptr(to_key), _ptr(_proj3(proj)), float(max_d),
                                           _ptr(tables), _ptr(n_faces), _ptr(active), _stream(vertices)), "bts_bbox_bounds")
    return tables, n_faces, active


def pseudo_depth(rays, grid, seg, tables, n_faces, active, semantic_id):
    """rays (ph * pw, 8), grid = (ph, pw), seg (hs, ws) fp32 labels -> (ph, pw): the z of the nearest valid intercept with the active
    boxes of the ray's label, +inf where there is none  (bts_bbox_pseudo_depth; evaluator_3dbb.py:102-128, :231-241)."""
    ph, pw = int(grid[0]), int(grid[1])
    _req(rays, "rays")
    rays = _req(rays.reshape(-1, 8), "rays", (ph * pw, 8))
    _req(seg, "seg")
    seg = _req(seg.reshape(seg.shape[-2:]), "seg")
    B = tables.shape[0]
    _req(tables, "tables", (B, M_MAX, 5)), _req(semantic_id, "semantic_id", (B,))
    _req_as(n_faces, "n_faces", torch.int32, (B,)), _req_as(active, "active", torch.uint8, (B,))      # as bbox_tables returns them
    out = torch.empty((ph, pw), device=rays.device, dtype=torch.float32)
    _lib.check(_lib.load().bts_bbox_pseudo_depth(_ptr(rays), ph, pw, _ptr(seg), seg.shape[0], seg.shape[1], _ptr(tables), _ptr(n_faces),
                                                 _ptr(active), _ptr(semantic_id), B, _ptr(out), _stream(rays)), "bts_bbox_pseudo_depth")
    return out


def metrics_from_counts(counts):
    """The nine metrics of evaluator_3dbb.py:288-299 from the six cell counts of bts_bbox_occupancy_eval (a seventh entry is ignored):
    _evalcommon.occupancy_ratios -- the ratios of lidar_occupancy.metrics_from_counts -- under this evaluator's names."""
    return dict(zip(METRIC_KEYS, occupancy_ratios(counts)))


class FusedBBoxOccupancyEval(FusedOccupancy):
    """BTSWrapper.forward of evaluator_3dbb.py around the render (:201-241, :253-299) in one library call.

        ev = FusedBBoxOccupancyEval(net)                   # an ENCODED behindthescenes_amd.BTSNet
        out = ev(bboxes, seg, rays, (ph, pw), pred_depth_z, proj, pose)
        out["o_acc"], out["no_nv_acc"], out["no_nv_rec"], ...

    The defaults are the evaluator's (:177-184).  ``bboxes`` is the data loader's list of box dicts (or the tuple pack_bboxes returns),
    ``seg`` the (hs, ws) label map, ``rays`` the (ph * pw, 8) key-frame rays of the half-resolution sampler, ``pred_depth_z`` (ph, pw)
    distance_to_z of their rendered depth (:251), ``proj`` the normalised (3, 3) intrinsics and ``pose`` the (4, 4) camera-to-world pose of
    the encoder view (projs[0, 0], poses[0, 0]).  Raises BtsNativeError when no box is active (the reference fails there too, :227)."""

    def __init__(self, net, x_range=(-4, 4), y_range=(0, 1), z_range=(20, 3), ppm=5, ppm_y=4, occ_threshold=0.5):
        self.occ_threshold, self.max_d = occ_threshold, z_range[0]
        grid, (self.xd, self.yd, self.zd) = get_pts(x_range, y_range, z_range, ppm, ppm_y)
        super().__init__(net, grid)

    def __call__(self, bboxes, seg, rays, grid, pred_depth_z, proj, pose, q_pts=None, want_masks=False, want_sigma=False,
                 want_pseudo_depth=False):
        ft = self._field()
        vertices, faces, semantic_id, v_off, f_off = bboxes if isinstance(bboxes, tuple) else pack_bboxes(bboxes)
        B = _req_boxes(vertices, faces, semantic_id, v_off, f_off, "FusedBBoxOccupancyEval")
        dev = vertices.device
        ph, pw = int(grid[0]), int(grid[1])
        _req(rays, "rays")
        rays = _req(rays.reshape(-1, 8), "rays", (ph * pw, 8))
        _req(seg, "seg")
        seg = _req(seg.reshape(seg.shape[-2:]), "seg")
        q = self._query(dev, q_pts)
        depth, K, pose = self._camera(pred_depth_z, proj, pose, (ph, pw))
        P = q.shape[0]
        counts, masks, sigma = self._outputs(dev, P, 7, want_masks, want_sigma)
        pseudo = torch.empty((ph, pw), device=dev, dtype=torch.float32) if want_pseudo_depth else None
        args = _lib.BtsBBoxOccupancyEval(q_pts=q.data_ptr(), P=P, B=B, ph=ph, pw=pw, hs=seg.shape[0], ws=seg.shape[1], vertices=vertices.data_ptr(),
                                         faces=faces.data_ptr(), v_offsets=C.cast(v_off, C.c_void_p).value,
                                         f_offsets=C.cast(f_off, C.c_void_p).value, semantic_id=semantic_id.data_ptr(), rays=rays.data_ptr(),
                                         seg=seg.data_ptr(), max_d=float(self.max_d), occ_threshold=float(self.occ_threshold),
                                         pred_depth_z=depth.data_ptr(), proj=K.data_ptr(), cam_pose=pose.data_ptr(), counts=counts.data_ptr(),
                                         masks=_addr(masks), sigma=_addr(sigma), pseudo_depth=_addr(pseudo), tables=None)
        self._launch("bts_bbox_occupancy_eval", ft, q, _lib.load().bts_bbox_occupancy_eval_workspace(P, B, ph, pw), args)
        host = counts.tolist()   # the ONE device-to-host copy
        if host[6] == 0:
            raise BtsNativeError(f"FusedBBoxOccupancyEval: none of the {B} boxes is in the frustum (no vertex within max_d = {self.max_d})")
        out = self._result(metrics_from_counts(host), host, masks, sigma)
        if want_pseudo_depth:
            out["pseudo_depth"] = pseudo
        return out
