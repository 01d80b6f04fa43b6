"""The LiDAR occupancy evaluation of the reference (models/bts/evaluator_lidar.py) on the HIP kernels of csrc/bts_occ.hip.

``get_pts``, ``get_lidar_slices`` and ``check_occupancy`` keep the reference's signatures and return types, so its evaluator binds with

    from behindthescenes_amd.lidar_occupancy import get_pts, get_lidar_slices, check_occupancy

``FusedOccupancyEval`` runs the whole frame after the render -- density query, LiDAR tables, occupancy vote, predicted visibility and
the counts behind the nine metrics -- from ONE library call (bts_occupancy_eval) and one device-to-host copy of six integers.
There is no torch fallback: CPU tensors are rejected, as everywhere else in this package."""
import ctypes as C
import math

import torch

from . import _lib, native
from ._evalcommon import FusedOccupancy, occupancy_ratios
from ._lib import BtsNativeError
from .native import _addr, _ptr, _req, _scratch, _stream

N_BINS = 360
METRIC_KEYS = ("o_acc", "o_rec", "o_prec", "ie_acc", "ie_rec", "ie_prec", "ie_r", "t_ie", "t_no_nop_nv")

_BORDERS = {}


def _borders(dev):
    """The 361 bin borders, built as the reference builds them (a CPU torch.linspace, evaluator_lidar.py:91) and kept per device."""
    b = _BORDERS.get(dev)
    if b is None:
        b = _BORDERS[dev] = torch.linspace(-math.pi, math.pi, N_BINS + 1).to(dev)
    return b


def get_pts(x_range, y_range, z_range, ppm, ppm_y, y_res=None):
    """The evaluator's query grid (evaluator_lidar.py:37-50): (y_res, z_res, x_res, 3) points on the CPU, x fastest, and the three sizes."""
    x_res = abs(int((x_range[1] - x_range[0]) * ppm))
    z_res = abs(int((z_range[1] - z_range[0]) * ppm))
    if y_res is None:
        y_res = abs(int((y_range[1] - y_range[0]) * ppm_y))
    ys = torch.tensor([y_range[0] * .5 + y_range[1] * .5]) if y_res == 1 else torch.linspace(y_range[0], y_range[1], y_res)
    xs, zs = torch.linspace(x_range[0], x_range[1], x_res), torch.linspace(z_range[0], z_range[1], z_res)
    grid = torch.empty((y_res, z_res, x_res, 3))
    grid[..., 0], grid[..., 1], grid[..., 2] = xs.view(1, 1, -1), ys.view(-1, 1, 1), zs.view(1, -1, 1)
    return grid, (x_res, y_res, z_res)


def _pack_clouds(point_clouds, velo_poses):
    clouds = list(point_clouds)
    T = len(clouds)
    if T == 0:
        raise BtsNativeError("get_lidar_slices: no point clouds")
    for k, pc in enumerate(clouds):
        _req(pc, f"point_clouds[{k}]")
        if pc.dim() != 2 or pc.shape[1] != 4:
            raise BtsNativeError(f"point_clouds[{k}]: expected (N, 4) homogeneous points, got {tuple(pc.shape)}")
    points = clouds[0] if T == 1 else torch.cat(clouds, dim=0)
    offsets = (C.c_int32 * (T + 1))()
    for k, pc in enumerate(clouds):
        offsets[k + 1] = offsets[k] + pc.shape[0]
    poses = torch.stack(list(velo_poses), dim=0) if not isinstance(velo_poses, torch.Tensor) else velo_poses
    poses = _req(poses.float().contiguous(), "velo_poses", (T, 4, 4))
    return points, offsets, poses, T


def lidar_tables(point_clouds, velo_poses, y_range, y_res, max_dist):
    """The one table tensor behind get_lidar_slices: (y_res, T, 362, 2) rows of (angle, distance)  (bts_lidar_slices)."""
    points, offsets, poses, T = _pack_clouds(point_clouds, velo_poses)
    lib = _lib.load()
    dev = points.device
    y_res = int(y_res)
    ws = _scratch(dev, lib.bts_lidar_slices_workspace(T, y_res))
    tables = torch.empty((max(y_res, 0), T, N_BINS + 2, 2), device=dev, dtype=torch.float32)
    _lib.check(lib.bts_lidar_slices(_ptr(points), offsets, T, _ptr(poses), _ptr(_borders(dev)), float(y_range[0]), float(y_range[-1]), y_res,
                                    float(max_dist), _ptr(ws), _ptr(tables), _stream(points)), "bts_lidar_slices")
    return tables


def get_lidar_slices(point_clouds, velo_poses, y_range, y_res, max_dist):
    """evaluator_lidar.py:57-115: a list over the y_res slices of lists over the clouds of (362, 2) tensors (angle, distance per 1 degree
    bin, with the two wrap rows) -- views of one table tensor."""
    tables = lidar_tables(point_clouds, velo_poses, y_range, y_res, max_dist)
    return [[tables[i, j] for j in range(tables.shape[1])] for i in range(tables.shape[0])]


def _tables_of(slices):
    """The (y_res, T, 362, 2) tensor the slices are views of, or a stacked copy when they are not."""
    y_res, T = len(slices), len(slices[0])
    first = slices[0][0]
    base = first._base if first._base is not None else None
    stride = (N_BINS + 2) * 2 * 4
    if (base is not None and tuple(base.shape) == (y_res, T, N_BINS + 2, 2) and base.is_contiguous() and base.dtype == torch.float32
            and all(len(s) == T for s in slices)
            and all(slices[i][j].data_ptr() == base.data_ptr() + (i * T + j) * stride for i in range(y_res) for j in range(T))):
        return base
    return torch.stack([torch.stack(list(s), dim=0) for s in slices], dim=0).float().contiguous()


def occupancy_masks(pts, tables, world_to_velo, min_dist=3):
    """pts (P, 3), tables (y_res, T, 362, 2), world_to_velo (T, 4, 4) -> is_occupied, is_visible as uint8 (P)  (bts_lidar_occupancy)."""
    _req(pts, "pts")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise BtsNativeError(f"pts: expected (P, 3), got {tuple(pts.shape)}")
    _req(tables, "tables")
    y_res, T = tables.shape[:2]
    _req(tables, "tables", (y_res, T, N_BINS + 2, 2)), _req(world_to_velo, "world_to_velo", (T, 4, 4))
    P = pts.shape[0]
    occ = torch.empty(P, device=pts.device, dtype=torch.uint8)
    vis = torch.empty(P, device=pts.device, dtype=torch.uint8)
    _lib.check(_lib.load().bts_lidar_occupancy(_ptr(pts), P, _ptr(tables), y_res, T, _ptr(world_to_velo), float(min_dist), _ptr(occ), _ptr(vis),
                                               _stream(pts)), "bts_lidar_occupancy")
    return occ, vis


def check_occupancy(pts, slices, velo_poses, min_dist=3):
    """evaluator_lidar.py:118-160: pts (P, 3) -> is_occupied (P) bool, is_visible (P) bool."""
    tables = _tables_of(slices)
    poses = torch.stack(list(velo_poses), dim=0) if not isinstance(velo_poses, torch.Tensor) else velo_poses
    world_to_velo = native.invert_small(poses)   # torch.inverse at :126
    occ, vis = occupancy_masks(pts.float().contiguous() if isinstance(pts, torch.Tensor) else pts, tables, world_to_velo, min_dist)
    return occ.view(torch.bool), vis.view(torch.bool)


def metrics_from_counts(counts):
    """The nine metrics of evaluator_lidar.py:319-340 from the six cell counts of bts_occupancy_eval: _evalcommon.occupancy_ratios under
    this evaluator's names."""
    return dict(zip(METRIC_KEYS, occupancy_ratios(counts)))


class FusedOccupancyEval(FusedOccupancy):
    """BTSWrapper.forward of evaluator_lidar.py after the render (:292-340) in one library call.

        ev = FusedOccupancyEval(net)                       # an ENCODED behindthescenes_amd.BTSNet
        out = ev(point_clouds, velo_poses, pred_depth_z, proj, pose)
        out["o_acc"], out["ie_acc"], out["ie_rec"], ...

    The defaults are the evaluator's (:220-231, :311-312).  ``pred_depth_z`` (H, W) is distance_to_z of the rendered depth (:289), ``proj``
    the normalised (3, 3) intrinsics and ``pose`` the (4, 4) camera-to-world pose of the encoder view (projs[0, 0], poses[0, 0])."""

    def __init__(self, net, x_range=(-4, 4), y_range=(0, .75), z_range=(20, 4), ppm=10, ppm_y=4, y_res=1, min_dist=3, occ_threshold=0.5,
                 max_dist=None):
        self.y_range, self.min_dist, self.occ_threshold = y_range, min_dist, occ_threshold
        self.max_dist = (z_range[0] ** 2 + x_range[0] ** 2) ** .5 if max_dist is None else max_dist
        grid, (self.xd, self.yd, self.zd) = get_pts(x_range, y_range, z_range, ppm, ppm_y, y_res)
        super().__init__(net, grid)

    def __call__(self, point_clouds, velo_poses, pred_depth_z, proj, pose, q_pts=None, want_masks=False, want_sigma=False, want_tables=False):
        ft = self._field()
        points, offsets, poses, T = _pack_clouds(point_clouds, velo_poses)
        dev = points.device
        q = self._query(dev, q_pts)
        depth, K, pose = self._camera(pred_depth_z, proj, pose)
        P, (H, W), y_res = q.shape[0], depth.shape, int(self.yd)
        counts, masks, sigma = self._outputs(dev, P, 6, want_masks, want_sigma)
        tables = torch.empty((y_res, T, N_BINS + 2, 2), device=dev, dtype=torch.float32) if want_tables else None
        args = _lib.BtsOccupancyEval(q_pts=q.data_ptr(), P=P, T=T, y_res=y_res, H=H, W=W, reserved_=0, points=points.data_ptr(),
                                     offsets=C.cast(offsets, C.c_void_p).value, velo_poses=poses.data_ptr(), borders361=_borders(dev).data_ptr(),
                                     y_lo=float(self.y_range[0]), y_hi=float(self.y_range[-1]), max_dist=float(self.max_dist),
                                     min_dist=float(self.min_dist), occ_threshold=float(self.occ_threshold), reserved2_=0,
                                     pred_depth_z=depth.data_ptr(), proj=K.data_ptr(), cam_pose=pose.data_ptr(), counts=counts.data_ptr(),
                                     masks=_addr(masks), sigma=_addr(sigma), tables=_addr(tables))
        self._launch("bts_occupancy_eval", ft, q, _lib.load().bts_occupancy_eval_workspace(P, T, y_res), args)
        host = counts.tolist()   # the ONE device-to-host copy
        out = self._result(metrics_from_counts(host), host, masks, sigma)
        if want_tables:
            out["tables"] = tables
        return out
