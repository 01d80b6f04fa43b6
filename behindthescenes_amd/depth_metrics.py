"""The depth evaluation of the reference (BTSWrapper.compute_depth_metrics, models/bts/evaluator.py:96-151; evaluator_nvs.py:96-139 is
the same function without scaling) on the HIP kernels of csrc/bts_depth_metrics.hip.

``compute_depth_metrics`` keeps the reference's shapes and keys, so its evaluator binds with

    from behindthescenes_amd.depth_metrics import compute_depth_metrics
    metrics = compute_depth_metrics(data["fine"][0]["depth"][:, :1], data["depths"][0], self.depth_scaling)

``FusedDepthEval`` runs the frame (``FusedEvalFrame``) and its metrics on one stream with nothing synchronised between them and keeps
one row per frame in a device buffer; ``compute()`` is the ONE device-to-host copy of an evaluation run.
There is no torch fallback: CPU tensors are rejected, as everywhere else in this package."""
import torch

from . import _lib, lidar_depth, native
from ._evalcommon import MetricRows
from ._lib import BtsNativeError
from .train_step import FusedEvalFrame

METRIC_KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")


def _frame(t, name):
    """(1, 1, H, W) -- or anything whose leading dimensions are 1 -- as a contiguous (1, H, W) view"""
    if not isinstance(t, torch.Tensor):
        raise BtsNativeError(f"{name}: expected a tensor")
    if t.dim() < 2 or t.numel() != t.shape[-2] * t.shape[-1]:
        raise BtsNativeError(f"{name}: one frame expected ((1, 1, H, W), the reference evaluates batch 1), got {tuple(t.shape)}")
    return t.reshape(1, t.shape[-2], t.shape[-1])


def _as_dict(row):
    return {k: row[i] for i, k in enumerate(METRIC_KEYS)}


def compute_depth_metrics(depth_pred, depth_gt, depth_scaling=None):
    """evaluator.py:96-151 on ``depth_pred (1, 1, H, W)`` and ``depth_gt (1, 1, Hg, Wg)``: the seven metrics as 0-dim device tensors
    (views of one row) under the reference's keys.  ``depth_scaling``: None, "median" or "l2".  Nothing synchronises."""
    row = native.depth_metrics(_frame(depth_pred, "depth_pred"), _frame(depth_gt, "depth_gt"), depth_scaling)[0]
    return _as_dict(row)


class FusedDepthEval(MetricRows):
    """An eval_depth frame that ends in one row of metrics on the device.

        ev = FusedDepthEval(wrapped, sampler, depth_scaling="median")
        for images, projs, poses, depth_gt in loader:
            data = ev.frame(images, projs, poses, depth_gt)      # the render dict of FusedEvalFrame + the seven metrics of this frame
        means = ev.compute()                                     # one device-to-host copy

    ``frame`` runs ``FusedEvalFrame`` and ``bts_depth_metrics`` on the same stream; the metrics read the frame's z-depth where the render
    wrote it and write row ``n_frames`` of a ``(capacity, 12)`` buffer.  ``compute`` returns, per metric, the mean over the frames seen
    as the reference's ``MeanMetric`` forms it: an fp64 sum of the per-frame values, frames whose value is NaN left out
    (utils/metrics.py:25-35).  Past ``capacity`` frames ``frame`` raises; it never wraps."""

    def __init__(self, wrapped, sampler, depth_scaling=None, capacity=4096):
        if depth_scaling not in native.DEPTH_SCALING_MODES:
            raise BtsNativeError(f"depth_scaling: expected None, 'median' or 'l2', got {depth_scaling!r}")
        super().__init__(_lib.BTS_DEPTH_METRICS_ROW, torch.float32, capacity, "FusedDepthEval")
        self.eval_frame = FusedEvalFrame(wrapped, sampler)
        self.depth_scaling = depth_scaling

    def update(self, depth_pred, depth_gt):
        """The metrics of one frame from a z-depth the caller already holds (``depth_pred (1, 1, H, W)``): the next row of the buffer."""
        self.full()
        pred, gt = _frame(depth_pred, "depth_pred"), _frame(depth_gt, "depth_gt")
        native._req(pred, "depth_pred"), native._req(gt, "depth_gt")
        row = self.next_row(pred.device)
        native.depth_metrics(pred, gt, self.depth_scaling, out=row)
        self.n_frames += 1
        return row[0]

    def frame(self, images, projs, poses, depth_gt, **kwargs):
        """``kwargs`` go to ``FusedEvalFrame.forward`` (ids_encoder, ids_render, jitter, ...); the depth must be the z-depth (to_z)."""
        if not kwargs.get("to_z", True):
            raise BtsNativeError("FusedDepthEval: the metrics are defined on the z-depth (to_z=True)")
        self.full()      # before the render, not after it
        native._req(_frame(depth_gt, "depth_gt"), "depth_gt")
        data = self.eval_frame(images, projs, poses, **kwargs)
        depth = data["fine"][0]["depth"]                 # (n, v, H, W); the reference takes [:, :1] of batch 1 (evaluator.py:99)
        if depth.shape[0] != 1:
            raise BtsNativeError(f"FusedDepthEval: the reference evaluates batch 1, this frame holds {depth.shape[0]} samples")
        row = self.update(depth[:, :1], depth_gt)
        data.update(_as_dict(row))
        data["depth_metrics_row"] = row
        return data

    def frame_lidar(self, images, projs, poses, points, P, convention, eigen_depth=False, size=None, **kwargs):
        """``frame`` with the ground truth formed here: ``points (N, 4)`` the frame's raw Velodyne cloud and ``P (3, 4)`` on the device,
        ``convention`` / ``eigen_depth`` as ``lidar_depth.load_depth`` takes them.  The map has the frame's size (the shipped configs
        evaluate at it) or ``size = (H, W)``; it is formed on the same stream, nothing synchronises, and it is returned as
        ``data["depth_gt"]`` (1, H, W) float32."""
        if size is None:
            if not isinstance(images, torch.Tensor) or images.dim() < 2:
                raise BtsNativeError("images: expected a tensor (n, v, 3, H, W)")
            size = tuple(images.shape[-2:])
        self.full()      # before any launch
        depth_gt = lidar_depth.load_depth(points, P, size, convention, eigen_depth)
        if depth_gt.dtype != torch.float32:
            depth_gt = depth_gt.float()      # the metrics are fp32, as the reference's after its data loader
        data = self.frame(images, projs, poses, depth_gt, **kwargs)
        data["depth_gt"] = depth_gt
        return data

    def compute(self):
        if self.n_frames == 0:
            raise BtsNativeError("FusedDepthEval.compute: no frame has been evaluated")
        return self.means(METRIC_KEYS)      # the ONE device-to-host copy
