"""A torch restatement of the reference's depth evaluation (BTSWrapper.compute_depth_metrics, models/bts/evaluator.py:96-151), written
from its behaviour: the nearest resize as an explicit index gather (the fp32 index formula PyTorch uses), the two masks, median / l2
scaling, the clamp, the per-pixel terms and their means.  dtype-generic (fp32 pins the kernels, fp64 arbitrates); runs on the CPU and,
eagerly, on the GPU (tools/depth_metrics_probe.py times it there with the reference's synchronisations).

``evaluate`` returns the per-pixel terms as well, so a caller can form the fp64 sum of the fp32 terms -- the quantity the kernels'
sums approximate to one fp32 rounding -- and takes optional ``coeffs=(x0, x1)`` that replace the scaling step (the l2 test evaluates
the terms with the kernel's own coefficients)."""
import torch

METRIC_KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
TERM_KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log")      # the terms whose means (and roots) the metrics of the same name are


def nearest_index(out_size, in_size, device="cpu"):
    """source index of every destination index: min((int)floorf(dst * scale), in - 1), scale = (float)in / (float)out, in fp32"""
    scale = torch.tensor(float(in_size), dtype=torch.float32) / torch.tensor(float(out_size), dtype=torch.float32)
    idx = torch.floor(torch.arange(out_size, dtype=torch.float32) * scale).to(torch.int64).clamp(max=in_size - 1)
    return idx.to(device)


def exact_index(out_size, in_size):
    """floor(dst * in / out) in integers: what the fp32 formula is NOT for some sizes"""
    return (torch.arange(out_size, dtype=torch.int64) * in_size // out_size).clamp(max=in_size - 1)


def resize_nearest(pred, Hg, Wg):
    """pred (..., H, W) -> (..., Hg, Wg) = F.interpolate(pred, (Hg, Wg)) (default mode nearest)"""
    iy, ix = nearest_index(Hg, pred.shape[-2], pred.device), nearest_index(Wg, pred.shape[-1], pred.device)
    return pred[..., iy, :][..., :, ix]


def evaluate(depth_pred, depth_gt, depth_scaling=None, coeffs=None, clamp=(1e-3, 80)):
    """depth_pred (1, 1, H, W), depth_gt (1, 1, Hg, Wg) -> dict:
    metrics (the seven 0-dim tensors), scale / shift (0-dim; 1 / 0 without scaling), counts [n_metric, n_scale, a1, a2, a3], terms (the
    per-pixel tensors behind abs_rel, sq_rel, rmse, rmse_log over the metric mask)."""
    depth_pred = resize_nearest(depth_pred, *depth_gt.shape[-2:])
    one, zero = torch.ones((), dtype=depth_pred.dtype, device=depth_pred.device), torch.zeros((), dtype=depth_pred.dtype, device=depth_pred.device)
    scale, shift = one, zero
    mask = depth_gt > 0
    if coeffs is not None:
        scale, shift = (torch.as_tensor(c, dtype=depth_pred.dtype, device=depth_pred.device) for c in coeffs)
        depth_pred = depth_pred * scale + shift
    elif depth_scaling == "median":
        scale = torch.median(depth_gt[mask]) / torch.median(depth_pred[mask])
        depth_pred = scale * depth_pred
    elif depth_scaling == "l2":
        A = torch.stack((depth_pred[mask], torch.ones_like(depth_pred[mask])), dim=-1)
        x = torch.linalg.lstsq(A.to(torch.float32), depth_gt[mask].unsqueeze(-1).to(torch.float32)).solution.squeeze()
        scale, shift = x[0], x[1]
        depth_pred = depth_pred * x[0] + x[1]
    elif depth_scaling is not None:
        raise ValueError(depth_scaling)
    n_scale = int(mask.sum())
    depth_pred = torch.clamp(depth_pred, clamp[0], clamp[1])
    mask = depth_gt != 0
    g, p = depth_gt[mask], depth_pred[mask]
    thresh = torch.maximum(g / p, p / g)
    hits = [thresh < 1.25, thresh < 1.25 ** 2, thresh < 1.25 ** 3]
    terms = dict(rmse=(g - p) ** 2, rmse_log=(torch.log(g) - torch.log(p)) ** 2, abs_rel=torch.abs(g - p) / g, sq_rel=((g - p) ** 2) / g)
    metrics = dict(abs_rel=terms["abs_rel"].mean(), sq_rel=terms["sq_rel"].mean(), rmse=terms["rmse"].mean() ** .5,
                   rmse_log=terms["rmse_log"].mean() ** .5, a1=hits[0].to(torch.float).mean(), a2=hits[1].to(torch.float).mean(),
                   a3=hits[2].to(torch.float).mean())
    counts = [int(mask.sum()), n_scale] + [int(h.sum()) for h in hits]
    return dict(metrics=metrics, scale=scale, shift=shift, counts=counts, terms=terms)


def metrics_from_terms64(terms, counts):
    """the seven metrics from the fp64 sums of the (fp32) terms: what a summation without rounding error gives"""
    n = counts[0]
    mean = {k: (terms[k].double().sum() / n if n else torch.tensor(float("nan"), dtype=torch.float64)) for k in TERM_KEYS}
    out = dict(abs_rel=mean["abs_rel"], sq_rel=mean["sq_rel"], rmse=mean["rmse"] ** .5, rmse_log=mean["rmse_log"] ** .5)
    for i, k in enumerate(("a1", "a2", "a3")):
        out[k] = torch.tensor(counts[2 + i] / n if n else float("nan"), dtype=torch.float64)
    return [float(out[k]) for k in METRIC_KEYS]
