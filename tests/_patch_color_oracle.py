"""CPU restatement in torch (fp32 or fp64, the inputs' dtype) of what csrc/bts_patch_color.hip and csrc/bts_loss_pixel_c.hip compute:
the 27 double-clamp colours of a point in a render view, the weighted sum along a ray, its gradient in the weights, and the
C-channel pixel loss.  Pinned against the real reference by tests/golden/gen_golden_patch_color.py (which also shows that the mutants
below leave the GPU test's bars) and tests/test_patch_color_cpu.py.

MUTANTS: one rule each changed, for the generator's power check --
  single_clamp   the coordinate is shifted by the patch offset and clamped once (not the texel);
  xy_order       the shifts are enumerated x-major: channel (x * 3 + y) * 3 + c;
  zero_padding   a shifted texel outside the frame contributes 0 instead of the clamped border texel;
  no_background  `composite` forgets 1 - sum(weights) under white_bkgd."""
import torch

from oracle import bts_oracle as O

CHANNELS = 27
MUTANTS = ("single_clamp", "xy_order", "zero_padding", "no_background")


def colours(imgs, w2c, Ks, xyz, mutant=None):
    """imgs (n, nv, 3, H, W) in [0, 1]: the processed RGB frames; w2c (n, nv, 4, 4), Ks (n, nv, 3, 3), xyz (n, P, 3)
    -> (n, P, nv, 27): channel (y * 3 + x) * 3 + c = sum_{a, b} w_ab imgs[c, clamp(y_a + y - 1), clamp(x_b + x - 1)] with the taps
    (y_a, x_b) and weights w_ab of grid_sample(bilinear, border, align_corners=False) at the point's projection."""
    n, nv, _, H, W = imgs.shape
    P = xyz.shape[1]
    xy, _, _, _ = O.project(xyz, w2c, Ks)                               # (n, nv, P, 2)
    flat = imgs.reshape(n, nv, 3, H * W)
    out = torch.zeros(n, nv, P, CHANNELS, dtype=imgs.dtype)
    for dy in range(3):
        for dx in range(3):
            sy, sx = dy - 1, dx - 1
            ix = ((xy[..., 0] + 1) * W - 1) / 2
            iy = ((xy[..., 1] + 1) * H - 1) / 2
            if mutant == "single_clamp":
                ix, iy = ix + sx, iy + sy
            ix, iy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
            fx, fy = ix.floor(), iy.floor()
            x0, y0 = fx.long(), fy.long()
            x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
            wx = ((fx + 1) - ix, ix - fx)
            wy = ((fy + 1) - iy, iy - fy)
            acc = None
            for a, ya in enumerate((y0, y1)):
                for b, xb in enumerate((x0, x1)):
                    r, c = (ya, xb) if mutant == "single_clamp" else (ya + sy, xb + sx)
                    inside = (r >= 0) & (r <= H - 1) & (c >= 0) & (c <= W - 1)
                    idx = r.clamp(0, H - 1) * W + c.clamp(0, W - 1)
                    tex = torch.gather(flat, 3, idx.unsqueeze(2).expand(-1, -1, 3, -1))      # (n, nv, 3, P)
                    if mutant == "zero_padding":
                        tex = tex * inside.unsqueeze(2).to(tex.dtype)
                    term = tex * (wx[b] * wy[a]).unsqueeze(2)
                    acc = term if acc is None else acc + term                                # nw, ne, sw, se: the kernels' order
            k = (dx * 3 + dy) if mutant == "xy_order" else (dy * 3 + dx)
            out[..., k * 3:k * 3 + 3] = acc.permute(0, 1, 3, 2)
    return out.permute(0, 2, 1, 3).contiguous()


def sample_colours(imgs, w2c, Ks, rays, z_samp, mutant=None):
    """rays (n * Bp, 8), z_samp (n * Bp, K) -> rgb_samps (n * Bp, K, nv * 27)"""
    n = imgs.shape[0]
    B, K = z_samp.shape
    pts = (rays[:, None, :3] + z_samp.unsqueeze(2) * rays[:, None, 3:6]).reshape(n, -1, 3)
    return colours(imgs, w2c, Ks, pts, mutant).reshape(B, K, -1)


def composite(weights, rgb_samps, white_bkgd, mutant=None):
    """weights (B, K), rgb_samps (B, K, nv * 27) -> rgb (B, nv * 27)  (nerf.py:298-304)"""
    rgb = (weights.unsqueeze(-1) * rgb_samps).sum(1)
    if white_bkgd and mutant != "no_background":
        rgb = rgb + 1 - weights.sum(1, keepdim=True)
    return rgb


def g_weights(g_rgb, rgb_samps, white_bkgd):
    """d (g_rgb . rgb) / d weights (B, K)"""
    g = (g_rgb.unsqueeze(1) * rgb_samps).sum(-1)
    return g - g_rgb.sum(-1, keepdim=True) if white_bkgd else g


def invalid_rays(policy, invalid, weights):
    """invalid (B, K, nv), weights (B, K) -> (B) bool  (loss.py:100-123)"""
    if policy == "strict":
        return torch.all(torch.any(invalid > .5, dim=-2), dim=-1)
    if policy == "weight_guided":
        return torch.all((invalid.to(weights.dtype) * weights.unsqueeze(-1)).sum(-2) > .9, dim=-1)
    return torch.zeros(invalid.shape[0], dtype=torch.bool)


def pixel_loss(rgb, rgb_gt, criterion, policy, invalid=None, weights=None):
    """rgb (B, nv, C), rgb_gt (B, C) -> (rgb term = mean over (B, C) of min_v crit * keep, its gradient in rgb, number of invalid rays)"""
    rgb = rgb.detach().clone().requires_grad_(True)
    d = rgb - rgb_gt.unsqueeze(1)
    e = (d.abs() if criterion == "l1" else d * d).amin(1)
    bad = invalid_rays(policy, invalid, weights) if policy not in (None, "none") else torch.zeros(rgb.shape[0], dtype=torch.bool)
    loss = (e * (1 - bad.to(e.dtype)).unsqueeze(-1)).mean()
    g, = torch.autograd.grad(loss, rgb)
    return loss.detach(), g, int(bad.sum())
