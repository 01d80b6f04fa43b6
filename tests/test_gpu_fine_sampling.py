"""GPU: the fine-pass sampling on its HIP kernel (bts_sample_fine, csrc/bts_sample_fine.hip; NeRFRenderer(native_fine_sampling=True))
against tests/golden/fine_sampling.npz -- the REAL reference's fp32 outputs, the same formulas in fp64 and the reference's own
distance D_z from them per layout (tests/golden/gen_golden_fine_sampling.py).  The bar is the project's usual one: at most twice as
far from the fp64 evaluation as the fp32 reference itself (2 * D_z, relative, sup norm); the depth draws are exact per operation and
must be the reference's bits.  The fixture has no draw within 8 * D_cdf of a cdf entry, so nothing is left out.

Measured on MI355X, the largest relative distance from fp64 of importance / merged / from-dist | the bar 2 * D_z:
    a_lin   4.756e-07 / 4.756e-07 / -          | 9.512e-07      a_dep   1.341e-07 / 1.341e-07 / -          | 2.681e-07
    b       9.784e-07 / 9.784e-07 / 1.755e-07  | 1.957e-06      c       1.551e-06 / 1.551e-06 / 1.797e-07  | 3.102e-06
    d_lin   9.687e-07 / 9.687e-07 / 1.330e-07  | 1.937e-06      d_dep   9.464e-08 / 9.464e-08 / 1.203e-07  | 2.406e-07
    d_clamp 1.032e-06 / 1.032e-06 / 1.556e-07  | 2.064e-06      e       -         / 5.262e-08 / -          | 1.052e-07
    protocol.npz  lin 4.592e-07 / - / 1.381e-07 | 9.185e-07     dep 1.298e-07 / - / 1.168e-07 | 2.596e-07
    end to end    fine pass 2.153e-07 | 4.306e-07 (1 of 1280 rays left out), from-dist 1.918e-07 | 3.837e-07 (none left out)
Every fixture output was bit-equal to the reference's fp32 value: the distances are the reference's own.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _fine_sampling_oracle as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "fine_sampling.npz"))
P = {k: torch.from_numpy(v) if v.dtype.kind == "f" else v for k, v in np.load(os.path.join(HERE, "golden", "protocol.npz")).items()}
LAYOUTS = ("a_lin", "a_dep", "b", "c", "d_lin", "d_dep", "d_clamp", "e")
DEPTH_STD = 0.5


@pytest.fixture(scope="module")
def hip():
    import behindthescenes_amd as bts
    from behindthescenes_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return bts


def case(tag):
    c = {k[len(tag) + 1:]: (torch.from_numpy(G[k]) if G[k].ndim else float(G[k])) for k in G.files if k.startswith(tag + "_")}
    B, Kc, Kf, Kfd, lindisp, n_dist = (int(x) for x in G[tag + "_meta"])
    c.update(B=B, Kc=Kc, Kf=Kf, Kfd=Kfd, lindisp=bool(lindisp), n_dist=n_dist)
    for k in ("u", "t", "noise"):
        c.setdefault(k, None)
    return c


def dev(c, *names):
    return [None if c[k] is None else c[k].cuda() for k in names]


def merged(native, c, count=None, z_coarse=None, depth=None):
    rays, w, zc, d, u, t, noise = dev(c, "rays", "weights", "z_coarse", "depth", "u", "t", "noise")
    return native.sample_fine(rays, w, zc if z_coarse is None else z_coarse, d if depth is None else depth, u, t, noise, DEPTH_STD, c["lindisp"],
                              nan_count=count)


def pieces(native, c, count=None):
    rays, w, d, u, t, noise = dev(c, "rays", "weights", "depth", "u", "t", "noise")
    return native.sample_fine(rays, w, None, d, u, t, noise, DEPTH_STD, c["lindisp"], nan_count=count)


def union64(c):
    return F.fine_union(c["rays"], c["weights"], c["z_coarse"], c["depth"], c["u"], c["t"], c["noise"], DEPTH_STD, c["lindisp"], torch.float64)


@pytest.mark.parametrize("tag", LAYOUTS)
def test_every_layout_and_mode_against_the_reference_fixture(hip, tag):
    native, c = hip.native, case(tag)
    bar = 2 * c["D_z"]
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    imp, dep = pieces(native, c, count)
    if c["u"] is not None:
        dist = F.rel_dist(imp.cpu(), c["f64_fine"])
        print(f"{tag}: importance {dist:.3e} (bar {bar:.3e}), bit-equal to the reference: {torch.equal(imp.cpu(), c['ref_fine'])}")
        assert imp.shape == c["ref_fine"].shape and dist <= bar
    else:
        assert imp is None
    if c["noise"] is not None:
        assert torch.equal(dep.cpu(), c["ref_fdepth"])          # exact per operation: the reference's bits
    else:
        assert dep is None
    z = merged(native, c, count).cpu()
    dist = F.rel_dist(z, union64(c))
    print(f"{tag}: merged {dist:.3e} (bar {bar:.3e}), bit-equal to the reference: {torch.equal(z, c['ref_union'])}")
    assert z.shape == (c["B"], c["Kc"] + c["Kf"]) and (z[:, 1:] >= z[:, :-1]).all()
    assert dist <= bar
    if c["n_dist"]:
        du, dt, w, zc = dev(c, "du", "dt", "weights", "z_coarse")
        zd = native.sample_coarse_from_dist(w, zc, du, dt, c["lindisp"], sort=True, nan_count=count).cpu()
        dist = F.rel_dist(zd, c["f64_dist"])
        print(f"{tag}: from-dist {dist:.3e} (bar {bar:.3e}), bit-equal to the reference: {torch.equal(zd, c['ref_dist'])}")
        assert zd.shape == (c["B"], c["n_dist"]) and (zd[:, 1:] >= zd[:, :-1]).all()
        assert dist <= bar
        # unsorted: the same values as drawn
        raw = native.sample_coarse_from_dist(w, zc, du, dt, c["lindisp"]).cpu()
        assert torch.equal(torch.sort(raw, dim=-1).values, zd)
    assert int(count.item()) == 0


@pytest.mark.parametrize("lindisp,tag", [(True, "lin"), (False, "dep")])
def test_the_protocol_fixture_layout_gets_the_same_bars(hip, lindisp, tag):
    """tests/golden/protocol.npz (B = 19, Kc = 8, n_fine = 6, n_fine_depth = 2, depth_std = 0.5): the reference's seeded CPU draws are
    reproduced as gen_golden_protocol.py made them (every draw is at least 4e-4 from a cdf entry)."""
    native = hip.native
    rays, w, depth, zc = P["smp_rays"], P["smp_weights"], P["smp_depth"], P[f"smp_{tag}_zc"]
    torch.manual_seed(6)
    du = torch.rand(19, 8)
    dt = torch.rand_like(du)
    torch.manual_seed(7)
    u = torch.rand(19, 4)
    t = torch.rand_like(u)
    torch.manual_seed(8)
    noise = torch.randn(19, 2)
    assert float(F.edge_distance(w, u).min()) > 1e-4 and float(F.edge_distance(w, du).min()) > 1e-4
    f64 = F.sample_fine(rays, w, u, t, lindisp, torch.float64)
    d64 = F.sample_coarse_from_dist(w, zc, du, dt, lindisp, torch.float64)
    D_z = max(F.rel_dist(P[f"smp_{tag}_fine"], f64), F.rel_dist(P[f"smp_{tag}_dist"], d64))
    imp, dep = native.sample_fine(rays.cuda(), w.cuda(), None, depth.cuda(), u.cuda(), t.cuda(), noise.cuda(), 0.5, lindisp)
    zd = native.sample_coarse_from_dist(w.cuda(), zc.cuda(), du.cuda(), dt.cuda(), lindisp)
    print(f"protocol {tag}: importance {F.rel_dist(imp.cpu(), f64):.3e}, from-dist {F.rel_dist(zd.cpu(), d64):.3e} (bar {2 * D_z:.3e})")
    assert F.rel_dist(imp.cpu(), f64) <= 2 * D_z and F.rel_dist(zd.cpu(), d64) <= 2 * D_z
    assert torch.equal(dep.cpu(), P[f"smp_{tag}_fdepth"])
    z = native.sample_fine(rays.cuda(), w.cuda(), zc.cuda(), depth.cuda(), u.cuda(), t.cuda(), noise.cuda(), 0.5, lindisp).cpu()
    z64 = F.fine_union(rays, w, zc, depth, u, t, noise, 0.5, lindisp, torch.float64)
    assert z.shape == (19, 14) and (z[:, 1:] >= z[:, :-1]).all() and F.rel_dist(z, z64) <= 2 * D_z


@pytest.mark.parametrize("tag", LAYOUTS)
def test_pieces_sorted_by_torch_are_the_merged_output(hip, tag):
    native, c = hip.native, case(tag)
    imp, dep = pieces(native, c)
    zc = c["z_coarse"].cuda()
    want = torch.sort(torch.cat([x for x in (zc, imp, dep) if x is not None], dim=-1), dim=-1).values
    assert torch.equal(merged(native, c), want)
    # z_coarse need not be sorted (a subclass may override sample_coarse)
    g = torch.Generator().manual_seed(1)
    shuffled = zc[:, torch.randperm(c["Kc"], generator=g).cuda()].contiguous()
    assert torch.equal(merged(native, c, z_coarse=shuffled), want)


@pytest.mark.parametrize("tag", ["a_lin", "c", "d_lin"])
def test_reruns_are_bit_identical_and_a_ragged_last_wave_stays_inside_its_buffer(hip, tag):
    """B is no multiple of the rays a wave (d: 8) or a work-group (a, c: 4) takes: the lanes behind the last ray must not store."""
    from behindthescenes_amd import _lib, native
    c = case(tag)
    rays, w, zc, d, u, t, noise = dev(c, "rays", "weights", "z_coarse", "depth", "u", "t", "noise")
    K, B = c["Kc"] + c["Kf"], c["B"]
    outs = []
    for _ in range(2):
        buf = torch.full((B * K + 4096,), -7.0, device="cuda")
        a = _lib.BtsSampleFineArgs(rays=rays.data_ptr(), weights=w.data_ptr(), z_coarse=zc.data_ptr(), depth=d.data_ptr(), u=u.data_ptr(), t=t.data_ptr(),
                                   noise=noise.data_ptr(), z_out=buf.data_ptr(), B=B, mode=0, Kc=c["Kc"], n_coarse=c["Kc"], Kf=c["Kf"], Kfd=c["Kfd"],
                                   lindisp=int(c["lindisp"]), sorted=1, depth_std=DEPTH_STD)
        _lib.check(_lib.load().bts_sample_fine(C.byref(a), native._stream(buf)), "bts_sample_fine")
        assert (buf[B * K:] == -7.0).all()
        outs.append(buf[:B * K].clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0].view(B, K), merged(native, c))


def test_nan_depth_is_counted_sorted_last_and_leaves_the_other_rays_alone(hip):
    native = hip.native
    c = case("d_lin")                 # eight rays per wave
    c["Kfd"], c["Kf"] = 2, 4
    g = torch.Generator().manual_seed(5)
    c["noise"] = torch.randn(c["B"], 2, generator=g)
    clean = merged(native, c)
    depth = c["depth"].clone()
    depth[10] = float("nan")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    z = merged(native, c, count, depth=depth.cuda())
    assert int(count.item()) == 2
    imp = pieces(native, c)[0]
    assert torch.isnan(z[10, -2:]).all() and torch.equal(z[10, :-2], torch.sort(torch.cat([c["z_coarse"][10].cuda(), imp[10]])).values)
    keep = torch.arange(c["B"], device="cuda") != 10
    assert torch.equal(z[keep], clean[keep])
    # the public method on its own keeps the reference's assert; the forward's counter raises once, then is clean
    r = hip.NeRFRenderer(n_coarse=c["Kc"], n_fine=4, n_fine_depth=2, lindisp=True, depth_std=DEPTH_STD, native_fine_sampling=True).cuda()
    rays = c["rays"].cuda()
    assert r.sample_fine_depth(rays, c["depth"].cuda(), noise=c["noise"].cuda()).shape == (c["B"], 2)
    with pytest.raises(AssertionError):
        r.sample_fine_depth(rays, depth.cuda(), noise=c["noise"].cuda())
    r.check_fine_samples()
    native.sample_fine(rays, c["weights"].cuda(), c["z_coarse"].cuda(), depth.cuda(), c["u"].cuda(), c["t"].cuda(), c["noise"].cuda(), DEPTH_STD, True,
                       nan_count=r.fine_nan_count)
    with pytest.raises(AssertionError):
        r.check_fine_samples()
    r.check_fine_samples()


@pytest.mark.parametrize("tag", ["d_lin", "d_dep"])
def test_draws_outside_the_cdf_and_nan_weights_follow_the_reference(hip, tag):
    """The quirks no fixture draw reaches, against torch's own searchsorted on the CPU (the restatement in fp32): a u above the last cdf
    entry gives ind = Kc and a depth outside [near, far] (no upper clamp), a u below 0 gives ind = 0, and a NaN weight makes every cdf
    entry "not above u" -- finite samples, nothing counted."""
    native, c = hip.native, case(tag)
    u, w = c["u"].clone(), c["weights"].clone()
    u[0::3, 0], u[1::3, 1] = 1.5, -0.5
    w[5, 2] = float("nan")
    want = F.sample_fine(c["rays"], w, u, c["t"], c["lindisp"])
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    imp, _ = native.sample_fine(c["rays"].cuda(), w.cuda(), None, None, u.cuda(), c["t"].cuda(), None, DEPTH_STD, c["lindisp"], nan_count=count)
    imp = imp.cpu()
    assert torch.equal(imp, want) and int(count.item()) == 0
    assert torch.isfinite(imp[5]).all() and ((imp[0::3, 0] > 80.0) | (imp[0::3, 0] < 3.0)).all()


@pytest.mark.parametrize("lindisp", [True, False])
def test_the_smallest_counts_sixteen_rays_to_a_wave(hip, lindisp):
    """Kc = 2, Kf = 1: K' = 4, sixteen rays per wave, B = 70 leaves the last wave ragged; draws at bin midpoints (bins at least 0.09 wide)"""
    native = hip.native
    g = torch.Generator().manual_seed(4)
    B = 70
    rays = torch.cat((torch.randn(B, 6, generator=g), torch.full((B, 1), 3.0), torch.full((B, 1), 80.0)), dim=-1)
    w = torch.rand(B, 2, generator=g) + 0.1
    zc = torch.sort(3.0 + 77.0 * torch.rand(B, 2, generator=g), dim=-1).values
    cdf = F.cdf_of(w, torch.float64)
    k = torch.randint(0, 2, (B, 1), generator=g)
    u = ((torch.gather(cdf, 1, k) + torch.gather(cdf, 1, k + 1)) / 2).float()
    t = torch.rand(B, 1, generator=g)
    z = native.sample_fine(rays.cuda(), w.cuda(), zc.cuda(), None, u.cuda(), t.cuda(), None, DEPTH_STD, lindisp).cpu()
    assert z.shape == (B, 3) and torch.equal(z, F.fine_union(rays, w, zc, None, u, t, None, DEPTH_STD, lindisp))


def test_two_pass_forward_with_native_fine_sampling_end_to_end(hip):
    """The scene of test_gpu_protocol.py::test_two_pass_forward_with_the_shared_mlp_end_to_end with native_fine_sampling and injected
    draws: the fine pass' samples against the CPU restatement fed the GPU's own coarse weights / depths / depth (2 * D_z, D_z the fp32
    restatement's own distance from fp64, computed here; rays with a draw within 8 * D_cdf of a cdf entry are left out, at most 2 % of
    them), the fine render of those samples against the oracle at that test's tolerances, gradients from both passes, and the
    sample_from_dist branch in the same way."""
    from oracle import bts_oracle as O
    from tests._cases import robust_ray_mask
    from tests._hip_helpers import build_net
    cfg = O.FieldConfig()
    g = torch.Generator().manual_seed(12)
    n, v, H, W, Kc, Kf, Kfd = 2, 3, 48, 160, 16, 12, 4
    scene = O.synthetic_scene(n, v, H, W, 64, seed=12, intrinsics=O.K_KITTI360, smooth=True)
    mlp = O.init_mlp(103, 64, 0, gen=g)
    rays = O.image_rays(scene["poses"], scene["projs"], H, W, 3.0, 80.0)
    rays = rays[:, torch.randperm(rays.shape[1], generator=g)[:640].sort().values].contiguous()
    net = build_net(cfg, mlp, scene, [1, 2], train=True)
    renderer = hip.NeRFRenderer.from_conf(dict(n_coarse=Kc, n_fine=Kf, n_fine_depth=Kfd, depth_std=1.0, lindisp=True, hard_alpha_cap=True,
                                               native_fine_sampling=True)).cuda().train()
    assert renderer.using_fine and renderer.native_fine_sampling
    B = n * 640
    u, t, noise = torch.rand(B, Kf - Kfd, generator=g), torch.rand(B, Kf - Kfd, generator=g), torch.randn(B, Kfd, generator=g)
    du, dt = torch.rand(B, Kc, generator=g), torch.rand(B, Kc, generator=g)
    renderer.fine_draws = dict(u=u.cuda(), t=t.cuda(), noise=noise.cuda(), dist_u=du.cuda(), dist_t=dt.cuda())
    wrapped = renderer.bind_parallel(net)
    torch.manual_seed(3)
    out = wrapped(rays.cuda(), want_weights=True, want_alphas=True, want_z_samps=True)
    assert set(out) == {"coarse", "fine"}
    flat = rays.reshape(-1, 8)
    st = O.make_state(scene, [1, 2], cfg)

    def check_samples(z_gpu, z32, z64, w, draws, what):
        D_cdf = float((F.cdf_of(w, torch.float32).double() - F.cdf_of(w, torch.float64)).abs().max())
        keep = ~(F.edge_distance(w, draws) < 8 * D_cdf).any(-1)
        D_z = F.rel_dist(z32[keep], z64[keep])
        dist = F.rel_dist(z_gpu[keep], z64[keep])
        print(f"{what}: {dist:.3e} (bar {2 * D_z:.3e}), {int((~keep).sum())} of {keep.numel()} rays left out, D_cdf {D_cdf:.2e}")
        assert float((~keep).float().mean()) <= 0.02
        assert (z_gpu[:, 1:] >= z_gpu[:, :-1]).all() and dist <= 2 * D_z

    def check_render(part, z):
        with torch.no_grad():
            ow, orgb, odepth, *_ = O.composite(flat, z, n, st, mlp, cfg, hard_alpha_cap=True)
        ok = robust_ray_mask(st, rays, z)
        torch.testing.assert_close(part["depth"].detach().cpu().reshape(-1)[ok], odepth[ok], rtol=1e-4, atol=0)
        torch.testing.assert_close(part["rgb"].detach().cpu().reshape(-1, 6)[ok], orgb[ok], rtol=0, atol=1e-5)
        torch.testing.assert_close(part["weights"].detach().cpu().reshape(-1, z.shape[-1])[ok], ow[ok], rtol=0, atol=1e-5)

    wc = out["coarse"]["weights"].detach().cpu().reshape(B, Kc)
    zc = out["coarse"]["z_samps"].detach().cpu().reshape(B, Kc)
    dc = out["coarse"]["depth"].detach().cpu().reshape(B)
    zf = out["fine"]["z_samps"].detach().cpu().reshape(B, Kc + Kf)
    args = (flat, wc, zc, dc, u, t, noise, 1.0, True)
    check_samples(zf, F.fine_union(*args), F.fine_union(*args, torch.float64), wc, u, "fine pass")
    check_render(out["fine"], zf)
    # gradients reach the MLP from each pass
    w_in = net.mlp_coarse.lin_in.weight
    for part in ("coarse", "fine"):
        gw, = torch.autograd.grad(out[part]["rgb"].square().mean() + 0.01 * out[part]["depth"].mean(), w_in, retain_graph=True)
        assert torch.isfinite(gw).all() and float(gw.abs().sum()) > 0, part
    renderer.check_fine_samples()
    # the sample_from_dist branch: the first pass' weights and depths as the proposal
    out3 = wrapped(rays.cuda(), want_weights=True, want_z_samps=True, sample_from_dist=(out["coarse"]["weights"].detach(), out["coarse"]["z_samps"].detach()))
    zd = out3["coarse"]["z_samps"].detach().cpu().reshape(B, Kc)
    d32 = torch.sort(F.sample_coarse_from_dist(wc, zc, du, dt, True), dim=-1).values
    d64 = torch.sort(F.sample_coarse_from_dist(wc, zc, du, dt, True, torch.float64), dim=-1).values
    check_samples(zd, d32, d64, wc, du, "from-dist")
    check_render(out3["coarse"], zd)
    renderer.check_fine_samples()
