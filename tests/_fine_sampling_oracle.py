"""CPU restatement of what sits between the two renders of NeRFRenderer.forward -- sample_fine, sample_fine_depth, the sorted union --
and of sample_coarse_from_dist (models/common/render/nerf.py:125-208, 356-367), with the draws as ARGUMENTS and the working precision
as a parameter: torch.float32 restates the reference operation by operation (tests/golden/gen_golden_fine_sampling.py checks that
against the real reference), torch.float64 is the yardstick the bars of tests/test_gpu_fine_sampling.py are measured from.

``mutant`` switches ONE of the reference's rules off; the fixture generator asserts that every mutant leaves the bars, i.e. that the
fixture can tell them apart:
    no_eps          no + 1e-5 on the weights
    div_kf          (ind + t) / Kf instead of / Kc
    depth_linear    the depth-linear near / far map under lindisp
    raw_borders     from-dist: the raw depths instead of the centred borders
    clamp_ns        from-dist: the interval clamped by ns - 1 instead of n_coarse - 1
    no_reciprocal   from-dist: no 1 / z on the way out under lindisp
"""
import torch

MUTANTS = ("no_eps", "div_kf", "depth_linear", "raw_borders", "clamp_ns", "no_reciprocal")


def cdf_of(weights, dtype=torch.float32, mutant=None):
    """weights (B, K) -> cdf (B, K + 1) = [0, cumsum(pdf)], pdf = (w + 1e-5) / sum(w + 1e-5)"""
    w = weights.detach().to(dtype)
    if mutant != "no_eps":
        w = w + 1e-5
    pdf = w / torch.sum(w, -1, keepdim=True)
    return torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)


def fine_inds(weights, u, dtype=torch.float32, mutant=None):
    """the bin of every importance draw: max(searchsorted(cdf, u, right=True) - 1, 0), (B, n) int64"""
    cdf = cdf_of(weights, dtype, mutant)
    return torch.clamp_min(torch.searchsorted(cdf, u.to(dtype).contiguous(), right=True) - 1, 0)


def near_far_map(rays, z_steps, lindisp, dtype=torch.float32):
    near, far = rays[:, -2:-1].to(dtype), rays[:, -1:].to(dtype)
    if not lindisp:
        return near * (1 - z_steps) + far * z_steps
    return 1 / (1 / near * (1 - z_steps) + 1 / far * z_steps)


def sample_fine(rays, weights, u, t, lindisp, dtype=torch.float32, mutant=None, n_fine=None):
    """rays (B, 8), weights (B, Kc), u, t (B, n) -> (B, n); n_fine: only the div_kf mutant reads it"""
    inds = fine_inds(weights, u, dtype, mutant).to(dtype)
    div = n_fine if mutant == "div_kf" else weights.shape[-1]
    z_steps = (inds + t.to(dtype)) / div
    return near_far_map(rays, z_steps, lindisp and mutant != "depth_linear", dtype)


def sample_fine_depth(rays, depth, noise, depth_std, dtype=torch.float32):
    """depth (B), noise (B, Kfd) -> (B, Kfd) = max(min(depth + noise * depth_std, far), near)"""
    z = depth.to(dtype).unsqueeze(1).repeat((1, noise.shape[1]))
    z = z + noise.to(dtype) * depth_std
    return torch.max(torch.min(z, rays[:, -1:].to(dtype)), rays[:, -2:-1].to(dtype))


def fine_union(rays, weights, z_coarse, depth, u, t, noise, depth_std, lindisp, dtype=torch.float32, mutant=None):
    """the fine pass' samples: sort([z_coarse | sample_fine | sample_fine_depth]) (nerf.py:356-367); u / noise None: that part is absent"""
    parts = [z_coarse.to(dtype)]
    n_fine = (0 if u is None else u.shape[1]) + (0 if noise is None else noise.shape[1])
    if u is not None:
        parts.append(sample_fine(rays, weights, u, t, lindisp, dtype, mutant, n_fine))
    if noise is not None:
        parts.append(sample_fine_depth(rays, depth, noise, depth_std, dtype))
    return torch.sort(torch.cat(parts, dim=-1), dim=-1).values


def dist_ids(weights, u, n_coarse, dtype=torch.float32, mutant=None):
    cdf = cdf_of(weights, dtype, mutant)
    hi = (weights.shape[-1] if mutant == "clamp_ns" else n_coarse) - 1
    return torch.clamp(torch.searchsorted(cdf, u.to(dtype).contiguous(), right=True) - 1, 0, hi)


def sample_coarse_from_dist(weights, z_samp, u, t, lindisp, dtype=torch.float32, mutant=None):
    """weights, z_samp (B, ns), u, t (B, n_coarse) -> (B, n_coarse), as drawn (the caller sorts)"""
    ids = dist_ids(weights, u, u.shape[1], dtype, mutant)
    z = z_samp.to(dtype)
    if lindisp:
        z = 1 / z
    if mutant == "raw_borders":
        borders = torch.cat((z, z[:, -1:]), dim=-1)
    else:
        centers = .5 * (z[:, 1:] + z[:, :-1])
        borders = torch.cat((z[:, :1], centers, z[:, -1:]), dim=-1)
    left, right = torch.gather(borders, -1, ids), torch.gather(borders, -1, ids + 1)
    interp = t.to(dtype)
    z_new = left * (1 - interp) + right * interp
    if lindisp and mutant != "no_reciprocal":
        z_new = 1 / z_new
    return z_new


def edge_distance(weights, u):
    """per draw, the distance (fp64) of u from the nearest cdf entry: (B, n)"""
    cdf = cdf_of(weights, torch.float64)
    return (u.to(torch.float64).unsqueeze(-1) - cdf.unsqueeze(1)).abs().min(-1).values


def rel_dist(a, b):
    """the largest relative distance of a from the fp64 yardstick b (NaNs on either side count as infinitely far)"""
    d = ((a.to(torch.float64) - b).abs() / b.abs()).max()
    return float("inf") if torch.isnan(d) else float(d)
