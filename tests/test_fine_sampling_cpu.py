"""CPU (no GPU, no launches): the host side of native_fine_sampling -- the renderer key and its draw seams, the generator consumption
with and without the key, bts_sample_fine's export, struct layout and every error path -- and the CPU restatement
(tests/_fine_sampling_oracle.py) against the fixtures of the REAL reference (fine_sampling.npz, protocol.npz)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import _lib, native
from behindthescenes_amd.build import build_library
from tests import _fine_sampling_oracle as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = np.load(os.path.join(HERE, "golden", "fine_sampling.npz"))
P = {k: torch.from_numpy(v) if v.dtype.kind == "f" else v for k, v in np.load(os.path.join(HERE, "golden", "protocol.npz")).items()}
LAYOUTS = ("a_lin", "a_dep", "b", "c", "d_lin", "d_dep", "d_clamp", "e")


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def _inputs(B=7, Kc=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    rays = torch.cat((torch.randn(B, 6, generator=g), torch.full((B, 1), 3.0), torch.full((B, 1), 80.0)), dim=-1)
    return rays, torch.rand(B, Kc, generator=g), torch.rand(B, generator=g) * 70 + 5, torch.sort(torch.rand(B, Kc, generator=g) * 70 + 4).values


def test_the_key_is_read_and_off_by_default_and_adds_nothing_to_the_state_dict():
    assert bts.NeRFRenderer.from_conf(dict(n_coarse=8)).native_fine_sampling is False
    assert bts.NeRFRenderer(n_coarse=8).native_fine_sampling is False
    r = bts.NeRFRenderer.from_conf(dict(n_coarse=8, n_fine=6, n_fine_depth=2, native_fine_sampling=True))
    assert r.native_fine_sampling is True and r.fine_draws is None
    assert r.fine_nan_count.dtype == torch.int32 and r.fine_nan_count.shape == (1,)
    assert set(r.state_dict()) == {"iter_idx", "last_sched"}            # the reference's checkpoint layout
    r.check_fine_samples()                                               # clean counter: nothing raised
    r.fine_nan_count += 3
    with pytest.raises(AssertionError):
        r.check_fine_samples()
    r.check_fine_samples()                                               # raised once, then clean


def test_without_the_key_the_methods_never_touch_the_new_entry(monkeypatch):
    def boom(*a, **kw):
        raise RuntimeError("the native entry was called without the key")
    monkeypatch.setattr(native, "sample_fine", boom)
    monkeypatch.setattr(native, "sample_coarse_from_dist", boom)
    rays, w, depth, zc = _inputs()
    r = bts.NeRFRenderer(n_coarse=8, n_fine=6, n_fine_depth=2, lindisp=True, depth_std=0.5)
    assert r.sample_fine(rays, w).shape == (7, 4) and r.sample_fine_depth(rays, depth).shape == (7, 2)
    assert r.sample_coarse_from_dist(rays, w, zc).shape == (7, 8)
    # the draw seams work without the key too, and give the restatement's values
    g = torch.Generator().manual_seed(3)
    u, t, noise = torch.rand(7, 4, generator=g), torch.rand(7, 4, generator=g), torch.randn(7, 2, generator=g)
    du, dt = torch.rand(7, 8, generator=g), torch.rand(7, 8, generator=g)
    assert torch.equal(r.sample_fine(rays, w, u=u, t=t), F.sample_fine(rays, w, u, t, True))
    assert torch.equal(r.sample_fine_depth(rays, depth, noise=noise), F.sample_fine_depth(rays, depth, noise, 0.5))
    assert torch.equal(r.sample_coarse_from_dist(rays, w, zc, u=du, t=dt), F.sample_coarse_from_dist(w, zc, du, dt, True))


def test_generator_consumption_is_the_same_with_and_without_the_key(monkeypatch):
    """draws that are not given are torch's, by the same calls in the same order with the same shapes (the native call is a stub here)"""
    calls = []

    def fake_fine(rays, weights, z_coarse, depth, u, t, noise, depth_std, lindisp, nan_count=None):
        calls.append(("fine", None if u is None else u.clone(), None if t is None else t.clone(), None if noise is None else noise.clone()))
        B = rays.shape[0]
        return (None if u is None else torch.zeros_like(u), None if noise is None else torch.zeros_like(noise)) if z_coarse is None else torch.zeros(B, 1)

    def fake_dist(weights, z_samp, u, t, lindisp, sort=False, nan_count=None):
        calls.append(("dist", u.clone(), t.clone(), None))
        return torch.zeros_like(u)
    monkeypatch.setattr(native, "sample_fine", fake_fine)
    monkeypatch.setattr(native, "sample_coarse_from_dist", fake_dist)
    rays, w, depth, zc = _inputs()
    states = {}
    for key in (False, True):
        r = bts.NeRFRenderer(n_coarse=8, n_fine=6, n_fine_depth=2, lindisp=True, depth_std=0.5, native_fine_sampling=key)
        st = []
        torch.manual_seed(11)
        r.sample_fine(rays, w), st.append(torch.get_rng_state())
        r.sample_fine_depth(rays, depth), st.append(torch.get_rng_state())
        r.sample_coarse_from_dist(rays, w, zc), st.append(torch.get_rng_state())
        states[key] = st
    for a, b in zip(states[False], states[True]):
        assert torch.equal(a, b)
    assert [c[0] for c in calls] == ["fine", "fine", "dist"]
    # ... and the stub was handed exactly the draws the torch composition consumes
    torch.manual_seed(11)
    u = torch.rand(7, 4)
    t = torch.rand_like(u)
    noise = torch.randn(7, 2)
    du = torch.rand(7, 8)
    dt = torch.rand_like(du)
    assert torch.equal(calls[0][1], u) and torch.equal(calls[0][2], t) and torch.equal(calls[1][3], noise)
    assert torch.equal(calls[2][1], du) and torch.equal(calls[2][2], dt)
    # given draws leave the generator alone
    r = bts.NeRFRenderer(n_coarse=8, n_fine=6, n_fine_depth=2, native_fine_sampling=True)
    before = torch.get_rng_state()
    r.sample_fine(rays, w, u=u, t=t), r.sample_fine_depth(rays, depth, noise=noise), r.sample_coarse_from_dist(rays, w, zc, u=du, t=dt)
    assert torch.equal(torch.get_rng_state(), before)


def test_cpu_tensors_are_a_native_error_as_everywhere_else():
    rays, w, depth, zc = _inputs()
    u = torch.rand(7, 4)
    with pytest.raises(bts.BtsNativeError):
        native.sample_fine(rays, w, zc, depth, u, u, torch.randn(7, 2), 0.5, True)
    with pytest.raises(bts.BtsNativeError):
        native.sample_coarse_from_dist(w, zc, torch.rand(7, 8), torch.rand(7, 8), True)
    r = bts.NeRFRenderer(n_coarse=8, n_fine=6, n_fine_depth=2, native_fine_sampling=True)
    with pytest.raises(bts.BtsNativeError):
        r.sample_fine(rays, w)


def test_the_entry_is_exported_and_its_struct_has_the_c_layout(lib):
    assert hasattr(lib, "bts_sample_fine") and "bts_sample_fine" in _lib.SYMBOLS and lib.bts_abi_version() == 9       # additive: ABI 9 stays
    fields = [f[0] for f in _lib.BtsSampleFineArgs._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bts_render.h"\nint main(void) {\n  printf("%zu\\n", sizeof(BtsSampleFineArgs));\n' + \
           "".join(f'  printf("%zu\\n", offsetof(BtsSampleFineArgs, {f}));\n' for f in fields) + \
           '  printf("%d %d\\n", BTS_SAMPLE_FINE, BTS_SAMPLE_FROM_DIST);\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.BtsSampleFineArgs)
    assert out[1:1 + len(fields)] == [getattr(_lib.BtsSampleFineArgs, f).offset for f in fields]
    assert out[-2:] == [_lib.BTS_SAMPLE_FINE, _lib.BTS_SAMPLE_FROM_DIST]


def test_every_error_path_has_its_code_and_message_and_launches_nothing(lib):
    def fine(**kw):
        a = dict(rays=16, weights=16, z_coarse=16, depth=16, u=16, t=16, noise=16, z_out=16, z_depth_out=16, B=4, mode=0, Kc=8, n_coarse=8, Kf=6,
                 Kfd=2, lindisp=1, sorted=1, depth_std=0.5)
        a.update(kw)
        return lib.bts_sample_fine(C.byref(_lib.BtsSampleFineArgs(**a)), None), lib.bts_last_error()

    def dist(**kw):
        return fine(**dict(dict(mode=1, Kc=8, n_coarse=8, Kf=0, Kfd=0), **kw))
    assert lib.bts_sample_fine(None, None) == -1 and b"NULL args" in lib.bts_last_error()
    for bad in (2, -1):
        rc, msg = fine(mode=bad)
        assert rc == -1 and b"unknown mode" in msg
    # non-positive sizes
    for kw in (dict(B=0), dict(Kc=0), dict(Kf=0, Kfd=0), dict(Kfd=-1), dict(B=-5)):
        rc, msg = fine(**kw)
        assert rc == -1 and b"non-positive size" in msg, kw
    for kw in (dict(B=0), dict(Kc=0), dict(n_coarse=0)):
        rc, msg = dist(**kw)
        assert rc == -1 and b"non-positive size" in msg, kw
    rc, msg = fine(Kf=2, Kfd=3)
    assert rc == -1 and b"Kfd = 3" in msg and b"Kf = 2" in msg
    rc, msg = dist(Kc=5, n_coarse=6)
    assert rc == -1 and b"n_coarse = 6" in msg and b"ns = 5" in msg
    # NULL required pointers: each one that the mode reads
    for name in ("rays", "weights", "u", "t", "depth", "noise", "z_out"):
        rc, msg = fine(**{name: None})
        assert rc == -1 and b"NULL required pointer" in msg, name
    for name in ("weights", "u", "t", "z_out", "z_depth_out"):         # pieces
        rc, msg = fine(z_coarse=None, **{name: None})
        assert rc == -1 and b"NULL required pointer" in msg, name
    for name in ("weights", "z_coarse", "u", "t", "z_out"):
        rc, msg = dist(**{name: None})
        assert rc == -1 and b"NULL required pointer" in msg, name
    # outside the envelope: BTS_E_UNSUPPORTED
    for kw in (dict(Kc=1), dict(Kc=200, Kf=57, Kfd=0), dict(Kc=256, Kf=1, Kfd=0), dict(B=(1 << 29) + 1)):
        rc, msg = fine(**kw)
        assert rc == -2 and (b"outside" in msg or b"2^29" in msg), kw
    for kw in (dict(Kc=1, n_coarse=1), dict(Kc=257, n_coarse=8), dict(B=(1 << 29) + 1)):
        rc, msg = dist(**kw)
        assert rc == -2, kw


@pytest.mark.parametrize("tag", LAYOUTS)
def test_the_restatement_is_the_reference_on_the_fixture(tag):
    c = {k[len(tag) + 1:]: (torch.from_numpy(G[k]) if G[k].ndim else float(G[k])) for k in G.files if k.startswith(tag + "_")}
    B, Kc, Kf, Kfd, lindisp, n_dist = (int(x) for x in G[tag + "_meta"])
    lindisp = bool(lindisp)
    u, t, noise = c.get("u"), c.get("t"), c.get("noise")
    assert c["rays"].shape == (B, 8) and c["weights"].shape == (B, Kc) and c["ref_union"].shape == (B, Kc + Kf)
    if u is not None:
        assert u.shape == (B, Kf - Kfd)
        # no near-ties: no draw within 8 * D_cdf of a cdf entry; fp32 and fp64 pick the same bins
        assert float(F.edge_distance(c["weights"], u).min()) >= 8 * c["D_cdf"]
        assert torch.equal(F.fine_inds(c["weights"], u, torch.float32), F.fine_inds(c["weights"], u, torch.float64))
        z = F.sample_fine(c["rays"], c["weights"], u, t, lindisp)
        torch.testing.assert_close(z, c["ref_fine"], rtol=1e-6, atol=0)
        assert F.rel_dist(z, c["f64_fine"]) <= 2 * c["D_z"]
        torch.testing.assert_close(F.sample_fine(c["rays"], c["weights"], u, t, lindisp, torch.float64), c["f64_fine"], rtol=1e-12, atol=0)
    if noise is not None:
        assert torch.equal(F.sample_fine_depth(c["rays"], c["depth"], noise, 0.5), c["ref_fdepth"])
        assert (c["ref_fdepth"] == 3.0).any() and (c["ref_fdepth"] == 80.0).any()          # both clamps bind
    z = F.fine_union(c["rays"], c["weights"], c["z_coarse"], c["depth"], u, t, noise, 0.5, lindisp)
    torch.testing.assert_close(z, c["ref_union"], rtol=1e-6, atol=0)
    assert F.rel_dist(c["ref_union"], F.fine_union(c["rays"], c["weights"], c["z_coarse"], c["depth"], u, t, noise, 0.5, lindisp, torch.float64)) <= c["D_z"]
    if n_dist:
        assert float(F.edge_distance(c["weights"], c["du"]).min()) >= 8 * c["D_cdf"]
        z = torch.sort(F.sample_coarse_from_dist(c["weights"], c["z_coarse"], c["du"], c["dt"], lindisp), dim=-1).values
        torch.testing.assert_close(z, c["ref_dist"], rtol=1e-6, atol=0)
        assert z.shape == (B, n_dist) and F.rel_dist(z, c["f64_dist"]) <= 2 * c["D_z"]
    # the fixture tells the mutants apart where they apply
    if u is not None:
        for m in ("no_eps", "div_kf") + (("depth_linear",) if lindisp else ()):
            assert F.rel_dist(F.sample_fine(c["rays"], c["weights"], u, t, lindisp, mutant=m, n_fine=Kf), c["f64_fine"]) > 2 * c["D_z"], m
    if n_dist:
        for m in ("raw_borders",) + (("no_reciprocal",) if lindisp else ()) + (("clamp_ns",) if n_dist < Kc else ()):
            z = torch.sort(F.sample_coarse_from_dist(c["weights"], c["z_coarse"], c["du"], c["dt"], lindisp, mutant=m), dim=-1).values
            assert F.rel_dist(z, c["f64_dist"]) > 2 * c["D_z"], m


@pytest.mark.parametrize("lindisp,tag", [(True, "lin"), (False, "dep")])
def test_the_restatement_is_the_reference_on_the_protocol_fixture(lindisp, tag):
    rays, w, depth, zc = P["smp_rays"], P["smp_weights"], P["smp_depth"], P[f"smp_{tag}_zc"]
    torch.manual_seed(6)
    du = torch.rand(19, 8)
    dt = torch.rand_like(du)
    torch.manual_seed(7)
    u = torch.rand(19, 4)
    t = torch.rand_like(u)
    torch.manual_seed(8)
    noise = torch.randn(19, 2)
    assert float(F.edge_distance(w, u).min()) >= 4e-4 and float(F.edge_distance(w, du).min()) >= 4e-4
    torch.testing.assert_close(F.sample_coarse_from_dist(w, zc, du, dt, lindisp), P[f"smp_{tag}_dist"], rtol=1e-6, atol=0)
    torch.testing.assert_close(F.sample_fine(rays, w, u, t, lindisp), P[f"smp_{tag}_fine"], rtol=1e-6, atol=0)
    assert torch.equal(F.sample_fine_depth(rays, depth, noise, 0.5), P[f"smp_{tag}_fdepth"])
