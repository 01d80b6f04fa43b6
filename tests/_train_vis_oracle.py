"""A torch restatement of what csrc/bts_train_vis.hip computes -- the eight panels of the trainer's ``visualize``
(models/bts/trainer.py:430-506) and the six scalar fields its colour map is applied to -- pinned by tests/golden/train_vis.npz, which
tests/golden/gen_golden_train_vis.py writes from the reference's own code.  ``evaluate(..., dtype=torch.float32)`` follows the
reference's operations one by one on float32 tensors (and reproduces its fields); ``dtype=torch.float64`` is the same mathematics on
doubles, the value the rounding errors of either fp32 evaluation are measured from.  ``mutant=`` names ONE deliberate misreading:

    entropy_ln_k        the entropy divided by ln K instead of log2 K
    alpha_sum_no_eps    the 1e-5 missing from the alpha sum
    profile_eps         the 1e-5 also in the profile
    profile_max_frame   the profile's maximum per frame instead of ONE over all 3 T rows
    rows_h_minus_1      the rows (h - 1) // 4, (h - 1) // 2, 3 (h - 1) // 4
    invalid_nv_only     the invalid mean over the views only (the K mean dropped: sample 0 stands for the ray)
    mse_no_half         the squared error not halved
    depth_clamp_first   the inverse depth clamped to [0, 1] before the normalisation instead of after it
"""
import math

import numpy as np
import torch

from tests._novel_views_oracle import cmap_index

MUTANTS = ("entropy_ln_k", "alpha_sum_no_eps", "profile_eps", "profile_max_frame", "rows_h_minus_1", "invalid_nv_only", "mse_no_half",
           "depth_clamp_first")
FIELDS = ("f_profile", "f_entropy", "f_alpha_sum", "f_mse", "f_invalid")        # plus f_depth_<s>
COLOURED = dict(depth_profile="f_profile", ray_entropy="f_entropy", alpha_sum="f_alpha_sum", recon_mse="f_mse", invalids="f_invalid")


# case z's special pixels (frame, y, x): see tests/golden/gen_golden_train_vis.py
Z_DEPTH_ZERO, Z_DEPTH_NAN, Z_ALPHAS_ZERO, Z_ALL_INVALID, Z_AGREE = (0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (0, 1, 2)


def decode(stored, v, agree=None):
    """the fixture's byte codes (first T frames) -> float32 inputs of ``v`` frames (frames from T on are copies of frame 0: nothing reads
    them): imgs (v, 3, h, w) = c / 127.5 - 1, rgb (v, h, w, nv, 3) = c / 255, alphas (v, h, w, K) = (c / 255)^2 with code 1 = -0.01,
    invalid (v, h, w, K, nv) = c / 255, depth (S, v, h, w) as stored.  ``agree`` (frame, y, x): that pixel's rgb is its image colour."""
    f32 = np.float32
    imgs = stored["imgs"].astype(f32) / f32(127.5) - f32(1)
    rgb = stored["rgb"].astype(f32) / f32(255)
    c = stored["alphas"].astype(f32) / f32(255)
    alphas = np.where(stored["alphas"] == 1, f32(-0.01), c * c).astype(f32)
    invalid = stored["invalid"].astype(f32) / f32(255)
    depth = np.array(stored["depth"], dtype=f32)
    if agree is not None:
        f, y, x = agree
        rgb[f, y, x] = (imgs[f, :, y, x] * f32(.5) + f32(.5))[None, :]
    T = imgs.shape[0]

    def pad(a, axis=0):
        if v == T:
            return np.ascontiguousarray(a)
        extra = np.repeat(np.take(a, [0], axis=axis), v - T, axis=axis)
        return np.ascontiguousarray(np.concatenate([a, extra], axis=axis))
    return dict(imgs=pad(imgs), rgb=pad(rgb), alphas=pad(alphas), invalid=pad(invalid), depth=pad(depth, 1))


def special_mask(field, shape, T):
    """case z: where a field holds a value that sits EXACTLY on a colour step by construction (compared exactly, not through the band)"""
    m = np.zeros(shape, dtype=bool)
    at = {"f_depth_0": [Z_DEPTH_ZERO, Z_DEPTH_NAN], "f_invalid": [Z_ALL_INVALID], "f_mse": [Z_AGREE]}.get(field, [])
    for p in at:
        m[p] = True
    return m


def coloured(S):
    """panel tag -> the field it colours"""
    out = {f"recon_depth_{s}": f"f_depth_{s}" for s in range(S)}
    out.update(COLOURED)
    return out


def profile_rows(h, mutant=None):
    return [(h - 1) // 4, (h - 1) // 2, 3 * (h - 1) // 4] if mutant == "rows_h_minus_1" else [h // 4, h // 2, 3 * h // 4]


def evaluate(imgs, rgb, depths, alphas, invalid, z_near, z_far, dtype=torch.float32, mutant=None):
    """imgs (v, 3, h, w), rgb (v, h, w, nv, 3), depths: S of (v, h, w), alphas (v, h, w, K), invalid (v, h, w, K, nv): float32 arrays of
    batch element 0; z_near, z_far numbers.  -> dict of numpy arrays of ``dtype``: input_im, recon_im (T, 3, h, w), f_depth_<s>
    (T, h, w), f_profile (3 T, K, w), f_entropy, f_alpha_sum, f_mse, f_invalid (T, h, w).  The inputs are not written."""
    assert mutant is None or mutant in MUTANTS, mutant
    t = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dtype)       # noqa: E731
    images, recon, alphas, invalid = t(imgs), t(rgb), t(alphas), t(invalid)
    # trainer.py:261-262: float32 tensors, whatever the config holds
    z_near, z_far = torch.tensor(float(z_near), dtype=torch.float32).to(dtype), torch.tensor(float(z_far), dtype=torch.float32).to(dtype)
    v, _, h, w = images.shape
    K = alphas.shape[-1]
    T = min(v, 6)
    out = {}
    with np.errstate(all="ignore"):
        images = images[:T] * .5 + .5
        recon = recon[:T].mean(dim=-2).permute(0, 3, 1, 2)
        out["input_im"], out["recon_im"] = images, recon
        sq = (images - recon) ** 2
        out["f_mse"] = (sq if mutant == "mse_no_half" else sq / 2).mean(dim=1).clamp(0, 1)
        for s, d in enumerate(depths):
            d = t(d)[:T]
            if mutant == "depth_clamp_first":
                out[f"f_depth_{s}"] = ((1 / d).clamp(0, 1) - 1 / z_far) / (1 / z_near - 1 / z_far)
            else:
                out[f"f_depth_{s}"] = ((1 / d - 1 / z_far) / (1 / z_near - 1 / z_far)).clamp(0, 1)
        eps = torch.tensor(1e-5, dtype=dtype)
        prof = alphas[:T][:, profile_rows(h, mutant), :, :]
        if mutant == "profile_eps":
            prof = prof + eps
        top = prof.reshape(T, -1).max(dim=1).values.view(T, 1, 1, 1) if mutant == "profile_max_frame" else prof.max()
        out["f_profile"] = (prof.clamp_min(0) / top).reshape(T * 3, w, K).permute(0, 2, 1)
        a = alphas[:T] + eps
        p = a / a.sum(dim=-1, keepdim=True)
        out["f_entropy"] = -(p * torch.log(p)).sum(-1) / (math.log(K) if mutant == "entropy_ln_k" else math.log2(K))
        out["f_alpha_sum"] = (alphas[:T] if mutant == "alpha_sum_no_eps" else a).sum(dim=-1) / K
        inv = invalid[:T]
        out["f_invalid"] = inv[..., 0, :].mean(-1) if mutant == "invalid_nv_only" else inv.mean(-2).mean(-1)
    return {k: x.contiguous().numpy() for k, x in out.items()}


def colour_indices(field32, N):
    """the table row of every element of a float32 field (matplotlib's rule)"""
    return cmap_index(np.asarray(field32, dtype=np.float32), N)


def panel_from_indices(idx, lut):
    """(..., h, w) row indices -> the (..., 3, h, w) channel-planar float64 panel the reference hands to make_grid"""
    lut = np.asarray(lut, dtype=np.float64)[:, :3]
    return np.moveaxis(lut[idx], -1, -3)


def panels(fields32, lut, S):
    """the coloured panels (float64, as the reference holds them) of fp32 ``fields32``"""
    N = np.asarray(lut).shape[0] - 3
    return {tag: panel_from_indices(colour_indices(fields32[f], N), lut) for tag, f in coloured(S).items()}


def near_step(field64, N, band):
    """where field64 * N lies within band * N of an integer: there an error of ``band`` may move the colour index by one"""
    x = np.asarray(field64, dtype=np.float64) * N
    with np.errstate(invalid="ignore"):
        return np.abs(x - np.round(x)) <= band * N
