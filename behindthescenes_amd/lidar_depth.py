"""The LiDAR ground-truth depth map of the reference's two KITTI data sets (``load_depth`` of datasets/kitti_raw/kitti_raw_dataset.py:
256-302 and of datasets/kitti_360/kitti_360_dataset.py:505-539) on the HIP kernels of csrc/bts_lidar_depth.hip: the producer of the
``depth_gt`` that ``compute_depth_metrics`` and ``FusedDepthEval.frame`` take.

The caller keeps the ``.bin`` read, the calibration and the split files and uploads the points; a data set binds with

    from behindthescenes_amd.lidar_depth import load_depth
    depth = load_depth(torch.from_numpy(points).cuda(), P_v2cl_on_device, BASE_SIZES[day], "kitti_raw", self.eigen_depth)

The rules -- last write wins, the off-by-one key that pairs ``(y, W - 1)`` with ``(y + 1, 0)``, round half to even -- are the
reference's and are listed in include/bts_render.h; the plain z-buffer is a different function.
There is no torch fallback: CPU tensors are rejected, as everywhere else in this package."""
import torch

from . import native

CONVENTIONS = ("kitti_raw", "kitti_360")


def load_depth_batch(points, offsets, P, size, convention, eigen_depth=False):
    """``B`` maps from one concatenated point array: ``points (N, 4)`` float32 on the device, ``offsets`` the ``B + 1`` host integers
    that cut it into clouds, ``P (3, 4)`` float32 or float64 on the device (kitti_raw's ``P_v2cl`` / kitti_360's
    ``K @ T_velo_to_cam[:3]``), ``size = (H, W)``.  Returns ``(B, 1, H, W)`` in ``P``'s dtype.  Nothing synchronises."""
    return native.lidar_depth(points, offsets, P, size, convention, eigen_depth).unsqueeze(1)


def load_depth(points, P, size, convention, eigen_depth=False):
    """One cloud: ``points (N, 4)`` float32 (the fourth column is taken as 1), ``P (3, 4)``, ``size = (H, W)``, ``convention``
    ``"kitti_raw"`` (with its ``eigen_depth``) or ``"kitti_360"``.  Returns ``(1, H, W)`` in ``P``'s dtype, the reference's shape."""
    n = points.shape[0] if isinstance(points, torch.Tensor) and points.dim() else 0
    return native.lidar_depth(points, (0, n), P, size, convention, eigen_depth)
