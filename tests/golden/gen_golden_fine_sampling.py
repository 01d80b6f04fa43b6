"""Golden fixture for the native fine-pass sampling (bts_sample_fine), produced by the REAL reference's NeRFRenderer (imported unmodified
through oracle/ref_shim.py; build container only):   python -B tests/golden/gen_golden_fine_sampling.py   -> fine_sampling.npz

Per layout (the smallest at which each regime of the kernel can go wrong; near = 3, far = 80):
    inputs   rays, weights, z_coarse, depth;  draws  u, t, noise, du, dt (stored explicitly: no test depends on a generator stream)
    ref_*    the reference's fp32 outputs: sample_fine, sample_fine_depth, the sorted union (nerf.py:356-367), sample_coarse_from_dist sorted
    f64_*    the same formulas in fp64 (tests/_fine_sampling_oracle.py)
             (the fp64 union is derived, not stored: the restatement's fine_union in fp64)
    D_cdf    the largest distance of the fp32 cdf from the fp64 cdf
    D_z      the largest relative distance of the reference's fp32 depths (all of the above) from the fp64 ones
The reference takes the stored draws through its own torch.rand / rand_like / randn_like calls (replaced by a queue while it runs).

No near-ties, by construction: a HIP cdf is not bit-equal to torch's, so every u within M = 8 * D_cdf of a cdf entry (fp64) is moved to
the midpoint of its ray's widest bin (at least 1 / Kc wide).  Asserted here, on the reference alone: none remain, at most 1 % were moved,
the fp32 and fp64 evaluations pick equal bins everywhere, the fp32 restatement IS the reference (1e-6), and each mutant of the restatement
leaves the 2 * D_z bar on at least one layout."""
import contextlib
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from oracle.ref_shim import load_reference
from tests import _fine_sampling_oracle as F

torch.set_num_threads(4)
NEAR, FAR, DEPTH_STD = 3.0, 80.0, 0.5
# tag: B, Kc, Kf, Kfd, lindisp, n_coarse of the from-dist run (0: none), a constructed narrow-bin block
LAYOUTS = {"a_lin": (130, 64, 40, 8, True, 0, True), "a_dep": (130, 64, 40, 8, False, 0, True),
           "b": (70, 48, 16, 0, True, 48, False), "c": (40, 160, 96, 16, True, 160, True),
           "d_lin": (33, 5, 3, 1, True, 5, False), "d_dep": (33, 5, 3, 1, False, 5, False), "d_clamp": (33, 5, 3, 1, True, 3, False),
           "e": (21, 16, 4, 4, False, 0, False)}


@contextlib.contextmanager
def injected(*draws):
    """torch.rand / rand_like / randn_like hand out `draws` in order while the reference runs"""
    queue = list(draws)
    saved = torch.rand, torch.rand_like, torch.randn_like

    def pop(*a, **kw):
        return queue.pop(0).clone()
    torch.rand = torch.rand_like = torch.randn_like = pop
    try:
        yield
    finally:
        torch.rand, torch.rand_like, torch.randn_like = saved
    assert not queue


def compositing_weights(g, B, K):
    """alpha = rand^8, the last alpha 1: peaked, many bins of width ~ 1e-5; one ray in eight all zero"""
    alpha = torch.rand(B, K, generator=g) ** 8
    alpha[:, -1] = 1.0
    trans = torch.cumprod(torch.cat([torch.ones(B, 1), 1 - alpha + 1e-10], -1), -1)[:, :-1]
    w = (alpha * trans).float()
    w[3::8] = 0.0
    return w


def settle(weights, u, narrow_rows):
    """moves the near-tie draws; -> u, D_cdf, the share moved"""
    D_cdf = float((F.cdf_of(weights, torch.float32).double() - F.cdf_of(weights, torch.float64)).abs().max())
    M = 8 * D_cdf
    cdf = F.cdf_of(weights, torch.float64)
    width, k = (cdf[:, 1:] - cdf[:, :-1]).max(-1)
    assert float(width.min()) >= 1 / weights.shape[1] - 1e-9
    mid = (torch.gather(cdf, 1, k[:, None]) + torch.gather(cdf, 1, k[:, None] + 1)) / 2
    near_tie = F.edge_distance(weights, u) < M
    u = torch.where(near_tie, mid.float().expand_as(u), u)
    assert not (F.edge_distance(weights, u) < M).any()
    if narrow_rows is not None:
        assert not near_tie[narrow_rows, 0].any()          # the constructed draws are the ones the search's precision is tested on
    share = float(near_tie.float().mean())
    assert share <= 0.01, share
    return u, D_cdf, share


def main():
    ref = load_reference()
    g = torch.Generator().manual_seed(2323)
    out, report = {}, {}
    cases = {}
    for tag, (B, Kc, Kf, Kfd, lindisp, n_dist, narrow) in LAYOUTS.items():
        n_imp = Kf - Kfd
        rays = torch.cat((torch.randn(B, 6, generator=g), torch.full((B, 1), NEAR), torch.full((B, 1), FAR)), dim=-1)
        w = compositing_weights(g, B, Kc)
        r = ref.NeRFRenderer(n_coarse=Kc, n_fine=Kf, n_fine_depth=Kfd, lindisp=lindisp, depth_std=DEPTH_STD)
        with injected(torch.rand(B, Kc, generator=g)):
            zc = r.sample_coarse(rays)
        depth = NEAR + (FAR - NEAR) * torch.rand(B, generator=g)
        depth[0::5], depth[1::5] = NEAR - 0.3, FAR + 0.3      # both clamps bind
        d = dict(rays=rays, weights=w, z_coarse=zc, depth=depth)
        D_cdf, rows = 0.0, None
        if n_imp:
            u, t = torch.rand(B, n_imp, generator=g), torch.rand(B, n_imp, generator=g)
            if narrow:
                # a block of 8 rays whose first draw sits at the midpoint of the ray's narrowest bin (width ~ 1e-5)
                rows = torch.tensor([i for i in range(B) if i % 8 != 3][:8])
                cdf = F.cdf_of(w[rows], torch.float64)
                k = (cdf[:, 1:] - cdf[:, :-1]).min(-1).indices
                u[rows, 0] = ((torch.gather(cdf, 1, k[:, None]) + torch.gather(cdf, 1, k[:, None] + 1)) / 2).float()[:, 0]
                assert float((cdf[:, 1:] - cdf[:, :-1]).min(-1).values.max()) < 2e-5
            u, D_cdf, share = settle(w, u, rows)
            with injected(u, t):
                fine = r.sample_fine(rays, w)
            assert torch.equal(F.fine_inds(w, u, torch.float32), F.fine_inds(w, u, torch.float64))
            f64 = F.sample_fine(rays, w, u, t, lindisp, torch.float64)
            torch.testing.assert_close(F.sample_fine(rays, w, u, t, lindisp), fine, rtol=1e-6, atol=0)
            d.update(u=u, t=t, ref_fine=fine, f64_fine=f64)
            report[tag] = dict(D_cdf=D_cdf, moved=share, D_z_fine=F.rel_dist(fine, f64))
        else:
            u = t = fine = None
        if Kfd:
            noise = torch.randn(B, Kfd, generator=g)
            with injected(noise):
                fdepth = r.sample_fine_depth(rays, depth)
            assert torch.equal(F.sample_fine_depth(rays, depth, noise, DEPTH_STD), fdepth)
            assert (fdepth == NEAR).any() and (fdepth == FAR).any() and ((fdepth > NEAR) & (fdepth < FAR)).any()
            d.update(noise=noise, ref_fdepth=fdepth)
        else:
            noise = fdepth = None
        # the fine pass' samples as the reference's forward forms them (nerf.py:356-367)
        union = torch.sort(torch.cat([x for x in (zc, fine, fdepth) if x is not None], dim=-1), dim=-1).values
        torch.testing.assert_close(F.fine_union(rays, w, zc, depth, u, t, noise, DEPTH_STD, lindisp), union, rtol=1e-6, atol=0)
        # (the fp64 union is not stored: it is sort([z_coarse | f64_fine | the restatement's fp64 depth draws]), F.fine_union in fp64)
        D_z = F.rel_dist(union, F.fine_union(rays, w, zc, depth, u, t, noise, DEPTH_STD, lindisp, torch.float64))
        d.update(ref_union=union)
        if n_dist:
            du, dt = torch.rand(B, n_dist, generator=g), torch.rand(B, n_dist, generator=g)
            du, D2, share = settle(w, du, None)
            D_cdf = max(D_cdf, D2)
            rd = ref.NeRFRenderer(n_coarse=n_dist, lindisp=lindisp)
            with injected(du, dt):
                dist = rd.sample_coarse_from_dist(rays, w, zc)
            assert torch.equal(F.dist_ids(w, du, n_dist, torch.float32), F.dist_ids(w, du, n_dist, torch.float64))
            torch.testing.assert_close(F.sample_coarse_from_dist(w, zc, du, dt, lindisp), dist, rtol=1e-6, atol=0)
            dist = torch.sort(dist, dim=-1).values                 # forward sorts it (nerf.py:340)
            f64 = torch.sort(F.sample_coarse_from_dist(w, zc, du, dt, lindisp, torch.float64), dim=-1).values
            d.update(du=du, dt=dt, ref_dist=dist, f64_dist=f64)
            D_z = max(D_z, F.rel_dist(dist, f64))
            report.setdefault(tag, {}).update(D_z_dist=F.rel_dist(dist, f64), moved_dist=share)
        if n_imp:
            D_z = max(D_z, F.rel_dist(fine, d["f64_fine"]))
        # D_z: the largest relative distance of ANY of the layout's fp32 reference depths from the fp64 ones -- the tests' bar is 2 * D_z
        d["D_cdf"], d["D_z"] = np.float64(D_cdf), np.float64(D_z)
        report.setdefault(tag, {}).update(D_z=D_z)
        d["meta"] = np.array([B, Kc, Kf, Kfd, int(lindisp), n_dist])
        cases[tag] = d
        out.update({f"{tag}_{k}": v for k, v in d.items()})
    # every mutant of the restatement leaves the 2 * D_z bar somewhere
    for m in F.MUTANTS:
        caught = []
        for tag, d in cases.items():
            B, Kc, Kf, Kfd, lindisp, n_dist = (int(x) for x in d["meta"])
            if "u" in d and m in ("no_eps", "div_kf", "depth_linear"):
                z = F.sample_fine(d["rays"], d["weights"], d["u"], d["t"], bool(lindisp), mutant=m, n_fine=Kf)
                if F.rel_dist(z, d["f64_fine"]) > 2 * float(d["D_z"]):
                    caught.append(tag)
            if n_dist and m in ("no_eps", "raw_borders", "clamp_ns", "no_reciprocal"):
                z = torch.sort(F.sample_coarse_from_dist(d["weights"], d["z_coarse"], d["du"], d["dt"], bool(lindisp), mutant=m), dim=-1).values
                if F.rel_dist(z, d["f64_dist"]) > 2 * float(d["D_z"]):
                    caught.append(tag + ":dist")
        assert caught, m
        report[f"mutant_{m}"] = caught
    path = os.path.join(HERE, "fine_sampling.npz")
    np.savez_compressed(path, **{k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print("fine_sampling.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")
    for k, v in report.items():
        print(" ", k, v)


if __name__ == "__main__":
    main()
