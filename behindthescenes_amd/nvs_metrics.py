"""The image half of the reference's novel-view-synthesis evaluation (BTSWrapper.compute_nvs_metrics, models/bts/evaluator_nvs.py:141-178)
on the HIP kernels of csrc/bts_nvs_metrics.hip: the nearest resize to eval_resolution, the 5 % crop, skimage's SSIM (7 x 7 uniform
window, fp64) and PSNR of the stereo / target view.  LPIPS (:171, an AlexNet forward with downloaded weights) stays with the caller.

``compute_nvs_metrics`` keeps the reference's shapes and keys, so its evaluator binds with

    from behindthescenes_amd.nvs_metrics import compute_nvs_metrics
    metrics = compute_nvs_metrics(data["fine"][0]["rgb"], data["rgb_gt"], self.eval_resolution)

``FusedNVSEval`` runs the frame (``FusedEvalFrame``), its image metrics and -- given a ground-truth depth -- the evaluator's depth
metrics (:96-139, ``bts_depth_metrics`` in mode none) on one stream with nothing synchronised between them and keeps one row per frame
in device buffers; ``compute()`` is the ONE device-to-host copy of an evaluation run.
There is no torch fallback: CPU tensors are rejected, as everywhere else in this package."""
import torch

from . import _lib, lidar_depth, native
from ._evalcommon import MetricRows, nan_skipping_means
from ._lib import BtsNativeError
from .depth_metrics import METRIC_KEYS as DEPTH_METRIC_KEYS, FusedDepthEval
from .train_step import FusedEvalFrame

METRIC_KEYS = ("ssim", "psnr")
ROW_KEYS = ("ssim", "psnr", "mse", "ssim_c0", "ssim_c1", "ssim_c2", "n_interior", "n_crop")


def _resolution(eval_resolution):
    try:
        h, w = (int(s) for s in eval_resolution)
    except (TypeError, ValueError):
        raise BtsNativeError(f"eval_resolution: (height, width) expected, got {eval_resolution!r}") from None
    if h <= 0 or w <= 0:
        raise BtsNativeError(f"eval_resolution: (height, width) expected, got {eval_resolution!r}")
    return h, w


def _views(rgb_pred, rgb_gt):
    """the stereo frame (:146-152) of ``rgb_pred (1, v, H, W, 1, 3)`` and ``rgb_gt (1, v, H, W, 3)`` as two (1, H, W, 3) views"""
    if not isinstance(rgb_pred, torch.Tensor) or not isinstance(rgb_gt, torch.Tensor):
        raise BtsNativeError("rgb_pred / rgb_gt: expected tensors")
    if rgb_gt.dim() != 5 or rgb_gt.shape[0] != 1 or rgb_gt.shape[-1] != 3:
        raise BtsNativeError(f"rgb_gt: (1, v, H, W, 3) expected (the reference evaluates batch 1), got {tuple(rgb_gt.shape)}")
    if rgb_pred.dim() != 6 or tuple(rgb_pred.shape) != tuple(rgb_gt.shape[:4]) + (1, 3):
        raise BtsNativeError(f"rgb_pred: {tuple(rgb_gt.shape[:4]) + (1, 3)} expected next to rgb_gt, got {tuple(rgb_pred.shape)}")
    sf_id = rgb_gt.shape[1] // 2                 # the target frame is always the "stereo" frame (:146)
    return rgb_pred[:, sf_id, :, :, 0], rgb_gt[:, sf_id]


def _as_dict(row):
    return {k: row[i] for i, k in enumerate(METRIC_KEYS)}


def compute_nvs_metrics(rgb_pred, rgb_gt, eval_resolution):
    """evaluator_nvs.py:141-170 on ``rgb_pred (1, v, H, W, 1, 3)`` (``data["fine"][0]["rgb"]``) and ``rgb_gt (1, v, H, W, 3)``
    (``data["rgb_gt"]``): ``ssim`` and ``psnr`` of view ``v // 2`` as 0-dim float64 device tensors (views of one row) under the
    reference's keys.  Both images are read where they lie; nothing synchronises."""
    pred, gt = _views(rgb_pred, rgb_gt)
    return _as_dict(native.nvs_metrics(pred, gt, _resolution(eval_resolution))[0])


class FusedNVSEval(MetricRows):
    """An eval_nvs frame that ends in one row of metrics on the device.

        ev = FusedNVSEval(wrapped, sampler, eval_resolution=(192, 640))
        for images, projs, poses, depth_gt in loader:
            data = ev.frame(images, projs, poses, depth_gt)      # the render dict of FusedEvalFrame + ssim, psnr (+ abs_rel ... a3)
        means = ev.compute()                                     # one device-to-host copy

    ``frame`` runs ``FusedEvalFrame`` with ``to_z=False`` (evaluator_nvs.py never calls ``distance_to_z``: its depth metrics run on the
    ray distance, reproduced here), ``bts_nvs_metrics`` on the stereo view where the render wrote it and, with ``depth_gt``,
    ``bts_depth_metrics`` in mode none, all on one stream; the rows go to a ``(capacity, 8)`` float64 and a ``(capacity, 12)`` float32
    buffer.  It serves ``eval_resolution`` equal to the frame size (the shipped data configs); a frame encoded at another resolution
    (``images_alt``) is the caller's render, followed by ``compute_nvs_metrics`` or ``update``.  ``compute`` returns, per metric, the
    mean over the frames seen as the reference's ``MeanMetric`` forms it: an fp64 sum of the per-frame values, frames whose value is NaN
    left out (utils/metrics.py:25-35); an infinite PSNR propagates.  Past ``capacity`` frames ``frame`` raises; it never wraps."""

    def __init__(self, wrapped, sampler, eval_resolution, capacity=4096):
        super().__init__(_lib.BTS_NVS_METRICS_ROW, torch.float64, capacity, "FusedNVSEval")
        self.eval_resolution = _resolution(eval_resolution)
        self.eval_frame = FusedEvalFrame(wrapped, sampler)
        self.depth = FusedDepthEval(wrapped, sampler, None, capacity=self.capacity)

    def reset(self):
        super().reset()
        self.depth.reset()

    def update(self, rgb_pred, rgb_gt):
        """The metrics of one frame from a render the caller already holds (the shapes of ``compute_nvs_metrics``): the next row."""
        self.full()
        pred, gt = _views(rgb_pred, rgb_gt)
        if not pred.is_cuda:
            raise BtsNativeError(f"rgb_pred: must live on the GPU (got {pred.device}); the HIP renderer has no CPU path")
        row = self.next_row(pred.device)
        native.nvs_metrics(pred, gt, self.eval_resolution, out=row)
        self.n_frames += 1
        return row[0]

    def frame(self, images, projs, poses, depth_gt=None, **kwargs):
        """``kwargs`` go to ``FusedEvalFrame.forward`` (ids_encoder, ids_render, jitter, ...); the depth stays the ray distance."""
        if kwargs.pop("to_z", False):
            raise BtsNativeError("FusedNVSEval: evaluator_nvs.py evaluates the ray distance (to_z=False)")
        if not isinstance(images, torch.Tensor) or images.dim() != 5 or tuple(images.shape[-2:]) != self.eval_resolution:
            size = tuple(images.shape[-2:]) if isinstance(images, torch.Tensor) and images.dim() >= 2 else None
            raise BtsNativeError(f"FusedNVSEval: eval_resolution {self.eval_resolution} is not the frame size {size}; render such a frame "
                                 "yourself (images_alt) and call compute_nvs_metrics / update on it")
        self.full()                              # before the render, not after it
        if depth_gt is not None:
            self.depth.full()
        data = self.eval_frame(images, projs, poses, to_z=False, **kwargs)
        row = self.update(data["fine"][0]["rgb"], data["rgb_gt"])
        data.update(_as_dict(row))
        data["nvs_metrics_row"] = row
        if depth_gt is not None:
            drow = self.depth.update(data["fine"][0]["depth"][:, :1], depth_gt)      # :98-99
            data.update({k: drow[i] for i, k in enumerate(DEPTH_METRIC_KEYS)})
            data["depth_metrics_row"] = drow
        return data

    def frame_lidar(self, images, projs, poses, points, P, convention, eigen_depth=False, size=None, **kwargs):
        """``frame`` with ``depth_gt`` formed on the same stream from the frame's raw Velodyne cloud (``lidar_depth.load_depth``: ``points
        (N, 4)`` and ``P (3, 4)`` on the device) at ``eval_resolution`` or ``size = (H, W)``; nothing synchronises.  The map is returned as
        ``data["depth_gt"]`` (1, H, W) float32."""
        self.full(), self.depth.full()           # before any launch
        depth_gt = lidar_depth.load_depth(points, P, self.eval_resolution if size is None else size, convention, eigen_depth)
        if depth_gt.dtype != torch.float32:
            depth_gt = depth_gt.float()
        data = self.frame(images, projs, poses, depth_gt, **kwargs)
        data["depth_gt"] = depth_gt
        return data

    def compute(self):
        if self.n_frames == 0:
            raise BtsNativeError("FusedNVSEval.compute: no frame has been evaluated")
        n_depth = self.depth.n_frames
        # the ONE device-to-host copy: the depth rows ride along as float64 (exact)
        both = self.rows[:self.n_frames, :len(METRIC_KEYS)].reshape(-1)
        if n_depth:
            both = torch.cat((both, self.depth.rows[:n_depth, :len(DEPTH_METRIC_KEYS)].double().reshape(-1)))
        host = both.cpu()
        parts = [(METRIC_KEYS, host[:self.n_frames * len(METRIC_KEYS)].reshape(self.n_frames, -1))]
        if n_depth:
            parts.append((DEPTH_METRIC_KEYS, host[self.n_frames * len(METRIC_KEYS):].reshape(n_depth, -1)))
        means = {}
        for keys, vals in parts:
            means.update(nan_skipping_means(vals, keys))
        return means
