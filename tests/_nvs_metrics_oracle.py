"""A restatement of the image half of the reference's NVS evaluation (BTSWrapper.compute_nvs_metrics, models/bts/evaluator_nvs.py:141-170),
written from its behaviour over the very primitive skimage calls: ``scipy.ndimage.uniform_filter(size=7)`` on float64 arrays and the
formulas of ``skimage.metrics.structural_similarity(win_size=7, gaussian_weights=False, data_range=R)`` and
``peak_signal_noise_ratio`` (skimage itself is no dependency of this project).  ``F.interpolate`` is an explicit gather through the fp32
index formula PyTorch uses, the crop box the reference's own Python expressions (:154-164).

Images are numpy arrays ``(H, W, 3)`` float32.  ``evaluate`` returns the row of bts_nvs_metrics: ssim psnr mse ssim_c0 ssim_c1 ssim_c2
n_interior n_crop.  Its keyword arguments are the mutants the fixture's generator holds the bars against (``cov_norm``, ``margin``, ``box``,
``dtype``); ``evaluate_direct`` is a second evaluation that sums every window directly, columns first."""
import math

import numpy as np
from scipy import ndimage

ROW_KEYS = ("ssim", "psnr", "mse", "ssim_c0", "ssim_c1", "ssim_c2", "n_interior", "n_crop")
WIN = 7


def nearest_index(out_size, in_size):
    """source index of every destination index: min((int)floorf(dst * scale), in - 1), scale = (float)in / (float)out, in fp32"""
    scale = np.float32(in_size) / np.float32(out_size)
    return np.minimum(np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64), in_size - 1)


def resize_nearest(img, He, We):
    """img (H, W, 3) -> (He, We, 3) = F.interpolate (default mode nearest) of the channel-first image (:154-155)"""
    return img[nearest_index(He, img.shape[0])][:, nearest_index(We, img.shape[1])]


def crop_box(He, We):
    """(y0, y1, x0, x1) of :158-161"""
    return int(math.ceil(0.05 * He)), int(math.floor(0.95 * He)), int(math.ceil(0.05 * We)), int(math.floor(0.95 * We))


def cropped(pred, gt, eval_resolution, box=None):
    He, We = eval_resolution
    y0, y1, x0, x1 = crop_box(He, We) if box is None else box
    return resize_nearest(pred, He, We)[y0:y1, x0:x1], resize_nearest(gt, He, We)[y0:y1, x0:x1]


def _row(ssim_c, mse, data_range, n_interior, n_crop):
    with np.errstate(divide="ignore"):
        psnr = 10 * np.log10(np.float64(data_range) ** 2 / mse)
    return np.array([np.mean(ssim_c), psnr, mse, *ssim_c, n_interior, n_crop], dtype=np.float64)


def _S(ux, uy, uxx, uyy, uxy, data_range, cov_norm):
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def evaluate(pred, gt, eval_resolution, data_range=1.0, cov_norm=WIN * WIN / (WIN * WIN - 1.0), margin=(WIN - 1) // 2, box=None, dtype=np.float64):
    return evaluate_cropped(*cropped(pred, gt, eval_resolution, box), data_range, cov_norm, margin, dtype)


def evaluate_cropped(x_all, y_all, data_range=1.0, cov_norm=WIN * WIN / (WIN * WIN - 1.0), margin=(WIN - 1) // 2, dtype=np.float64):
    """:169-170 on the two cropped (h, w, 3) images the reference hands to skimage"""
    h, w = x_all.shape[:2]
    if min(h, w) < WIN:
        raise ValueError("win_size exceeds image extent")          # skimage's refusal
    # peak_signal_noise_ratio: both images as float64, the mean over every element
    mse = np.mean((x_all.astype(np.float64) - y_all.astype(np.float64)) ** 2, dtype=np.float64)
    ssim_c = []
    for c in range(3):
        x, y = x_all[..., c].astype(dtype), y_all[..., c].astype(dtype)
        ux, uy, uxx, uyy, uxy = (ndimage.uniform_filter(a, size=WIN) for a in (x, y, x * x, y * y, x * y))
        S = _S(ux, uy, uxx, uyy, uxy, dtype(data_range), dtype(cov_norm))
        ssim_c.append(np.mean(S[margin:h - margin, margin:w - margin], dtype=np.float64))
    return _row(ssim_c, mse, data_range, (h - 2 * margin) * (w - 2 * margin), h * w)


def evaluate_direct(pred, gt, eval_resolution, data_range=1.0):
    """the same quantities with every window summed directly (down its columns, then across), no running sums"""
    x_all, y_all = cropped(pred, gt, eval_resolution)
    h, w = x_all.shape[:2]
    x_all, y_all = x_all.astype(np.float64), y_all.astype(np.float64)
    d = (x_all - y_all).transpose(2, 1, 0).reshape(-1)
    mse = math.fsum(d * d) / d.size
    ssim_c = []
    for c in range(3):
        x, y = x_all[..., c], y_all[..., c]

        def win_mean(a):
            v = np.lib.stride_tricks.sliding_window_view(a, (WIN, WIN))       # (h - 6, w - 6, 7, 7)
            return v.sum(axis=2).sum(axis=2) / (WIN * WIN)
        S = _S(win_mean(x), win_mean(y), win_mean(x * x), win_mean(y * y), win_mean(x * y), data_range, WIN * WIN / (WIN * WIN - 1.0))
        ssim_c.append(math.fsum(S.reshape(-1)) / S.size)
    return _row(ssim_c, mse, data_range, (h - WIN + 1) * (w - WIN + 1), h * w)


def inputs_g():
    """case g, 192 x 640 at identity: a closed-form pattern as ground truth, the prediction that pattern shifted by a fifth of a period
    plus seeded uniform noise -- regenerated, not stored.  Only +, -, *, abs and the remainder of doubles are used, and the generator's
    uniform draw: every machine forms the same bits (no libm call whose last bit may differ)."""
    H, W = 192, 640
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    yy, xx, ch = yy[..., None], xx[..., None], np.arange(3, dtype=np.float64)

    def tri(t):          # a triangle wave of period 1 in [-1, 1]
        return 2.0 * np.abs(2.0 * np.remainder(t, 1.0) - 1.0) - 1.0
    gt = 0.5 + 0.3 * tri(0.0175 * xx + 0.11 * ch) * tri(0.011 * yy - 0.06 * ch) + 0.1 * tri(0.0014 * xx * yy / 8.0)
    rng = np.random.default_rng(20261018)
    pred = 0.5 + 0.3 * tri(0.0175 * xx + 0.11 * ch + 0.2) * tri(0.011 * yy - 0.06 * ch) + 0.1 * (2.0 * rng.random((H, W, 3)) - 1.0)
    return np.clip(pred, 0, 1).astype(np.float32), np.clip(gt, 0, 1).astype(np.float32)
