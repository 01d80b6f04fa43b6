"""What the evaluators share, each written once: the nine occupancy ratios (lidar_occupancy, bbox_occupancy), the frame of the two fused
occupancy evaluators, and the row accumulator with the reference's NaN-skipping mean (depth_metrics, nvs_metrics).  Private: the public
names stay in the evaluators' own modules."""
import ctypes as C

import torch

from . import _lib, native
from ._lib import BtsNativeError
from .native import _ptr, _req, _scratch, _stream


def occupancy_ratios(counts):
    """The nine values of evaluator_lidar.py:319-340 (= evaluator_3dbb.py:288-299) from the six cell counts
    [V&P, V&!P, !V&O&P, !V&O&!P, !V&!O&P, !V&!O&!P] (further entries are ignored), in the order of both modules' METRIC_KEYS:
    o_acc, o_rec, o_prec, ie_acc, ie_rec, ie_prec, ie_r, t_ie, t_no_nop_nv.  Types as in the reference: Python floats where it calls
    .item(), 0-dim fp32 tensors (here on the CPU) elsewhere; a mean over an empty selection is NaN, as torch's mean of an empty tensor."""
    c = [int(v) for v in counts][:6]

    def ratio(num, den):
        return torch.tensor(float(num), dtype=torch.float32) / torch.tensor(float(den), dtype=torch.float32)

    n = sum(c)
    return (ratio(c[1] + c[2] + c[5], n).item(), ratio(c[2], c[2] + c[3]).item(), ratio(c[2], c[0] + c[2] + c[4]).item(),
            ratio(c[2] + c[5], c[2] + c[3] + c[4] + c[5]).item(), ratio(c[5], c[4] + c[5]), ratio(c[5], c[3] + c[5]),
            ratio(c[4] + c[5], n).item(), float(c[4] + c[5]), torch.tensor(float(c[5]), dtype=torch.float32))


def proj3(proj):
    """the normalised intrinsics as a contiguous (3, 3)"""
    _req(proj, "proj")
    return _req(proj.reshape(proj.shape[-2:])[:3, :3].contiguous(), "proj", (3, 3))


class FusedOccupancy:
    """The frame of FusedOccupancyEval and FusedBBoxOccupancyEval: the query grid kept per device, the checks of the field, the query
    points and the camera, the outputs, the library call with fresh scratch, the result's tail.  Each evaluator's __call__ adds what is
    its own (clouds and tables / boxes, labels and rays) and fills its argument struct."""

    def __init__(self, net, grid):
        self.net = net
        self._q_cpu = grid.reshape(-1, 3).contiguous()
        self._q = None

    def q_pts(self, dev):
        if self._q is None or self._q.device != dev:
            self._q = self._q_cpu.to(dev)
        return self._q

    def _field(self):
        who, ft = type(self).__name__, self.net.native_field()
        if isinstance(ft, native.MultiViewField):
            raise BtsNativeError(f"{who}: not available for a field with more than one encoder view")
        if ft.mlp_color:
            raise BtsNativeError(f"{who}: not available for MLP-predicted colour (sample_color=False)")
        if ft.n != 1:
            raise BtsNativeError(f"{who}: the evaluator queries one encoded sample, this field holds {ft.n}")
        native._check_partial(ft, None, None, who)
        return ft

    def _query(self, dev, q_pts):
        q = _req(self.q_pts(dev) if q_pts is None else q_pts, "q_pts")
        if q.dim() != 2 or q.shape[1] != 3:
            raise BtsNativeError(f"q_pts: expected (P, 3), got {tuple(q.shape)}")
        return q

    @staticmethod
    def _camera(pred_depth_z, proj, pose, shape=None):
        """-> the predicted z-depth as (H, W) (``shape``, when given), the (3, 3) intrinsics, the (4, 4) pose"""
        depth = _req(pred_depth_z.reshape(pred_depth_z.shape[-2:]) if isinstance(pred_depth_z, torch.Tensor) else pred_depth_z, "pred_depth_z", shape)
        K = proj3(proj)
        _req(pose, "pose")
        return depth, K, _req(pose.reshape(4, 4), "pose", (4, 4))

    @staticmethod
    def _outputs(dev, P, n_counts, want_masks, want_sigma):
        return (torch.empty(n_counts, device=dev, dtype=torch.int32), torch.empty((3, P), device=dev, dtype=torch.uint8) if want_masks else None,
                torch.empty(P, device=dev, dtype=torch.float32) if want_sigma else None)

    def _launch(self, entry, ft, q, ws_bytes, args):
        ws = _scratch(q.device, ws_bytes)
        cfg, tens = ft.cfg(), ft.tensors(self.net.mlp_coarse.packed().detach())
        with torch.no_grad():
            _lib.check(getattr(_lib.load(), entry)(C.byref(cfg), C.byref(tens), C.byref(args), _ptr(ws), ws_bytes, _stream(q)), entry)

    @staticmethod
    def _result(out, host, masks, sigma):
        out["counts"] = host
        if masks is not None:
            out["is_occupied_pred"], out["is_occupied"], out["is_visible"] = (m.view(torch.bool) for m in masks)
        if sigma is not None:
            out["sigma"] = sigma
        return out


def nan_skipping_means(vals, keys):
    """{key: mean of column i of the fp64 host tensor ``vals``} as the reference's MeanMetric forms it (utils/metrics.py:25-35): an fp64
    sum over the rows that are not NaN, divided by their number; NaN when there is none; an infinite value propagates."""
    keep = ~torch.isnan(vals)
    sums, n = torch.where(keep, vals, torch.zeros_like(vals)).sum(dim=0), keep.sum(dim=0)
    return {k: (sums[i].item() / int(n[i]) if int(n[i]) else float("nan")) for i, k in enumerate(keys)}


class MetricRows:
    """One row of ``row_len`` values per frame in a ``(capacity, row_len)`` device buffer (``rows``, allocated on the first frame's
    device; ``n_frames`` of it are filled).  Past ``capacity`` rows ``full`` / ``next_row`` raise; nothing wraps."""

    def __init__(self, row_len, dtype, capacity, who):
        if int(capacity) <= 0:
            raise BtsNativeError(f"capacity: a positive number of frames expected, got {capacity}")
        self.row_len, self.dtype, self.capacity, self.who = int(row_len), dtype, int(capacity), who
        self.rows, self.n_frames = None, 0

    def reset(self):
        if self.rows is not None:
            self.rows.zero_()
        self.n_frames = 0

    def full(self, what="frames"):
        if self.n_frames >= self.capacity:
            raise BtsNativeError(f"{self.who}: {self.capacity} {what} are stored; compute() / reset() first or construct with a larger capacity")

    def next_row(self, device):
        """The (1, row_len) view the next frame's metrics go to (a buffer on another device starts over); the writer counts it:
        ``n_frames += 1`` once the row is written."""
        self.full()
        if self.rows is None or self.rows.device != device:
            self.rows = torch.zeros((self.capacity, self.row_len), device=device, dtype=self.dtype)
            self.n_frames = 0
        return self.rows[self.n_frames:self.n_frames + 1]

    def means(self, keys):
        """nan_skipping_means of the first len(keys) columns of the filled rows: one device-to-host copy"""
        return nan_skipping_means(self.rows[:self.n_frames, :len(keys)].cpu().double(), keys)
