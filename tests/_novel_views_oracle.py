"""A numpy restatement of what csrc/bts_frames.hip computes -- color_tensor (utils/plotting.py:41-46 on matplotlib's Colormap.__call__),
the statements of render_poses after the render (scripts/inference_setup.py:189-196) and the scripts' normalisation / uint8 lines
(scripts/videos/gen_vid_nvs.py:105-120) -- pinned by tests/golden/novel_views.npz, which tests/golden/gen_golden_novel_views.py
writes from the reference's own code.  The keyword switches are the MUTANTS the generator shows to change the fixture's outputs:
``fold=False`` (t == N not folded to N - 1), ``nan_bad=False`` (NaN not mapped to the bad colour), ``threshold64=True`` (0.8 compared as
a double), ``max_after=True`` (the frame maximum taken after masking, i.e. over the valid pixels).  ``u8_fp32=True`` (x 255 in fp32) is
kept as a switch although it is no mutant: it gives the same byte for every float32 in [0, 1], which the generator asserts."""
import numpy as np

F32 = np.float32


def cmap_index(x, N, fold=True, nan_bad=True):
    """matplotlib's index of a float32 array: xa *= N in fp32; xa == N -> N - 1; < 0 -> N (under); >= N -> N + 1 (over); NaN -> N + 2
    (bad); otherwise a truncation"""
    t = np.asarray(x, dtype=F32) * F32(N)
    if fold:
        t = np.where(t == F32(N), F32(N - 1), t)
    under, over, bad = t < 0, t >= N, np.isnan(t)
    with np.errstate(invalid="ignore"):
        idx = np.where(bad | under | over, F32(0), t).astype(np.int64)
    idx[under], idx[over] = N, N + 1
    idx[bad] = N + 2 if nan_bad else 0
    return idx


def normalise(x):
    """(x - min) / (max - min) in fp32 with the image's own extrema; a NaN anywhere makes both extrema NaN (torch's min() / max())"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        lo, hi = (F32(np.nan), F32(np.nan)) if np.isnan(x).any() else (x.min(), x.max())
        return ((x - lo) / (hi - lo)).astype(F32)


def colorize(x, lut, norm=False, **mutant):
    """one image ``x (...)`` -> (..., 3) float64 from ``lut (N + 3, 3 | 4)``"""
    lut = np.asarray(lut, dtype=np.float64)[:, :3]
    if norm:
        x = normalise(x)
    return lut[cmap_index(x, lut.shape[0] - 3, **mutant)]


def lut_u8(lut):
    return (np.asarray(lut, dtype=np.float64)[:, :3] * 255).astype(np.uint8)


def colorize_u8(x, lut, norm=False, **mutant):
    if norm:
        x = normalise(x)
    return lut_u8(lut)[cmap_index(x, np.asarray(lut).shape[0] - 3, **mutant)]


def to_u8(v, u8_fp32=False):
    """(v * 255).astype(uint8) on the float64 concatenation of gen_vid_nvs.py:110-120, saturated, NaN -> 0"""
    v = np.asarray(v, dtype=F32)
    t = (v * F32(255)).astype(np.float64) if u8_fp32 else v.astype(np.float64) * 255.0
    t = np.where(np.isnan(t), 0.0, t)
    return np.clip(np.trunc(t), 0, 255).astype(np.uint8)


def norm_range(d_min, d_max):
    """1 / d_max and the denominator as Python evaluates them, rounded once to fp32"""
    return F32(1 / d_max), F32(1 / d_min - 1 / d_max)


def finish(rgb, depth, wsum, d_min, d_max, lut, black_invalid, threshold64=False, max_after=False, u8_fp32=False, **mutant):
    """rgb (h, w, 3), depth (h, w), wsum (h, w) float32 -> dict(rgb, depth: the masked floats; img_u8, depth_u8: (h, w, 3) panels;
    invalid)"""
    rgb, depth, wsum = np.array(rgb, dtype=F32), np.array(depth, dtype=F32), np.asarray(wsum, dtype=F32)
    invalid = (wsum.astype(np.float64) > 0.8) if threshold64 else (wsum > F32(0.8))
    if black_invalid:
        top = depth[~invalid].max() if (max_after and (~invalid).any()) else depth.max()
        depth[invalid] = top
        rgb[invalid] = 0
    a, den = norm_range(d_min, d_max)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = ((F32(1) / depth - a) / den).astype(F32)
    t = np.where(t < 0, F32(0), np.where(t > 1, F32(1), t))          # clamp(0, 1): a NaN stays a NaN
    return dict(rgb=rgb, depth=depth, invalid=invalid, img_u8=to_u8(rgb, u8_fp32), depth_u8=colorize_u8(t, lut, **mutant))
