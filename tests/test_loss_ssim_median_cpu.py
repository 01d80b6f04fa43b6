"""CPU (no GPU, no kernel launches): the opt-in `native_ssim_median: true` of ReconstructionLoss -- criterion l1+ssim WITH
median_thresholding: what constructs with the key and what still refuses, the C ABI of bts_photometric_loss_median (exports, every
BTS_E_INVALID path with its message before anything is read or launched), BtsNativeError instead of a CPU fallback, and the CPU
restatement tests/_loss_ssim_median_oracle.py, mutants included, against tests/golden/loss_ssim_median.npz (the REAL reference's
ReconstructionLoss: tests/golden/gen_golden_loss_ssim_median.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import _lib
from behindthescenes_amd.build import build_library
from tests import _loss_ssim_median_oracle as MO

E_INVALID = -1
KEY = {"native_ssim_median": True}
BASE = dict(criterion="l1+ssim", median_thresholding=True)


@pytest.fixture(scope="module")
def lib():
    build_library()          # hipcc cross-compiles for gfx950 without a GPU
    return _lib.load()


@pytest.mark.parametrize("policy", ["none", None, "strict", "weight_guided"])
def test_with_the_key_ssim_median_constructs(policy):
    crit = bts.ReconstructionLoss(dict(BASE, invalid_policy=policy, lambda_edge_aware_smoothness=0.01, **KEY))
    assert crit.native_ssim_median and crit.ssim_median and crit.median_thresholding and crit.criterion_str == "l1+ssim"
    assert crit.get_loss_metric_names() == ["loss", "loss_rgb_coarse", "loss_rgb_fine", "loss_ray_entropy", "loss_depth_reg"]


def test_with_the_key_diverse_and_automasking_construct_with_their_own_keys():
    bts.ReconstructionLoss(dict(BASE, invalid_policy="weight_guided_diverse", native_pixel_loss=True, **KEY))
    crit = bts.ReconstructionLoss(dict(BASE, invalid_policy="weight_guided", native_automask=True, **KEY), use_automasking=True)
    assert crit.use_automasking and crit.ssim_median
    bts.ReconstructionLoss(dict(BASE, invalid_policy="weight_guided_diverse", native_pixel_loss=True, native_automask=True, **KEY), use_automasking=True)
    with pytest.raises(NotImplementedError, match="native_pixel_loss: true"):
        bts.ReconstructionLoss(dict(BASE, invalid_policy="weight_guided_diverse", **KEY))
    with pytest.raises(NotImplementedError, match="native_automask: true"):
        bts.ReconstructionLoss(dict(BASE, **KEY), use_automasking=True)


def test_without_the_key_construction_still_raises_and_names_the_key():
    for conf in (dict(BASE), dict(BASE, native_ssim_median=False), dict(BASE, invalid_policy="weight_guided", native_pixel_loss=True),
                 dict(BASE, invalid_policy="weight_guided_diverse", native_pixel_loss=True)):
        with pytest.raises(NotImplementedError, match=r"'l1\+ssim' with median_thresholding=True") as e:
            bts.ReconstructionLoss(conf)
        assert "native_ssim_median: true" in str(e.value) and "coefficient gather" not in str(e.value)
    with pytest.raises(NotImplementedError, match="native_ssim_median: true"):
        bts.ReconstructionLoss(dict(BASE, native_pixel_loss=True, native_automask=True), use_automasking=True)


def test_the_key_alone_changes_nothing_else():
    crit = bts.ReconstructionLoss(dict(criterion="l1+ssim", invalid_policy="weight_guided", **KEY))
    assert not crit.ssim_median
    with pytest.raises(NotImplementedError, match="native_pixel_loss: true"):
        bts.ReconstructionLoss(dict(criterion="l1", median_thresholding=True, **KEY))


def test_symbols_export_and_the_abi_version_stays(lib):
    for name in ("bts_photometric_loss_median", "bts_photometric_loss_median_workspace"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.bts_abi_version() == _lib.ABI_VERSION == 9
    assert C.sizeof(_lib.BtsLossArgs) == 120 and _lib.BtsLossArgs.invalid_any.offset == 112      # the shipped struct keeps its layout
    assert bts.native.photometric_loss_median


def test_workspace_size_is_positive_monotone_and_above_the_tiled_one(lib):
    ws = lib.bts_photometric_loss_median_workspace
    assert ws(8, 8, 8, 3, 2) > 0 and ws(1, 192, 640, 1, 1) > 0
    for bad in ((0, 8, 8, 3, 1), (8, 0, 8, 3, 1), (8, 8, 0, 3, 1), (8, 8, 8, 0, 1), (8, 8, 8, 3, 0), (8, 8, 8, 3, 3), (-8, 8, 8, 3, 2)):
        assert ws(*bad) == 0, bad
    for a, b in (((8, 8, 8, 3, 2), (16, 8, 8, 3, 2)), ((8, 8, 8, 3, 2), (8, 8, 8, 3, 4)), ((2, 40, 72, 1, 1), (4, 40, 72, 1, 1)),
                 ((1024, 8, 8, 4, 16), (2048, 8, 8, 4, 16))):
        assert ws(*a) <= ws(*b), (a, b)
    # the tiled layout with the gradient factors, plus one float per ray, plus 24 KB of histograms per batch sample
    for (P, h, w, nv, n) in ((8, 8, 8, 3, 2), (4, 20, 36, 2, 2), (1, 40, 72, 1, 1)):
        tiled = lib.bts_photometric_loss_tiled_automask_workspace(P, h, w, nv)
        assert ws(P, h, w, nv, n) >= tiled + 4 * P * h * w + n * 3 * 2048 * 4


def _args(P=8, ph=8, pw=8, nv=3, K=4, policy=1, eas=1, **ptrs):
    """A BtsLossArgs whose pointers are non-NULL dummies: the calls below must fail before anything is read or launched."""
    d = dict(rgb=16, depth=16, weights=16, invalid=16, rgb_gt=16, parts=16, g_rgb=None, g_depth=None, invalid_wsum=None, invalid_any=None)
    d.update(ptrs)
    return _lib.BtsLossArgs(n_patches=P, patch_h=ph, patch_w=pw, nv=nv, K=K, invalid_policy=policy, edge_aware_smoothness=eas, scale_rgb=1.0,
                            scale_eas=1.0, **d)


def test_argument_errors_are_codes_with_messages(lib):
    need = lib.bts_photometric_loss_median_workspace(8, 8, 8, 3, 2)
    assert need > 0

    def call(a, n=2, out=16, ws=16, nbytes=need):
        return lib.bts_photometric_loss_median(C.byref(a) if a is not None else None, n, None, out, None, None, ws, nbytes, None)
    err = lambda: lib.bts_last_error()
    assert call(None) == E_INVALID and b"bts_photometric_loss_median" in err() and b"NULL required pointer" in err()
    for k in ("rgb", "rgb_gt", "parts", "depth"):
        assert call(_args(**{k: None})) == E_INVALID and b"NULL required pointer" in err() and b"bts_photometric_loss_median" in err(), k
    assert call(_args(), out=None) == E_INVALID and b"NULL required pointer" in err()
    assert call(_args(depth=None, eas=0), nbytes=0) == E_INVALID and b"workspace too small" in err()      # depth is only needed with smoothness
    for n in (0, -2):
        assert call(_args(), n=n) == E_INVALID and b"non-positive size" in err() and b"bts_photometric_loss_median" in err(), n
    for k in ("P", "ph", "pw", "nv"):
        assert call(_args(**{k: 0})) == E_INVALID and b"non-positive size" in err(), k
        assert call(_args(**{k: -3})) == E_INVALID and b"non-positive size" in err(), k
    assert call(_args(), n=3) == E_INVALID and b"not a multiple of n = 3" in err() and b"bts_photometric_loss_median" in err()
    for p in (-1, 3):
        assert call(_args(policy=p)) == E_INVALID and b"unknown invalid_policy" in err(), p
    assert call(_args(policy=1, invalid=None)) == E_INVALID and b"invalid_policy 1 needs" in err()
    assert call(_args(policy=1, K=0)) == E_INVALID and b"invalid_policy 1 needs" in err()
    assert call(_args(policy=2, weights=None)) == E_INVALID and b"invalid_policy 2 needs" in err()
    assert call(_args(policy=2, invalid=None)) == E_INVALID and b"invalid_policy 2 needs" in err()
    assert call(_args(P=1 << 20, ph=64, pw=64), n=1) == E_INVALID and b"2^31 - 1 rays" in err()
    assert call(_args(), nbytes=need - 1) == E_INVALID and b"workspace too small" in err() and b"bts_photometric_loss_median_workspace" in err()
    assert call(_args(), ws=None) == E_INVALID and b"workspace too small" in err()
    # the per-ray reductions stand in for the per-sample rows (checked, then the workspace check refuses: still nothing launched)
    assert call(_args(policy=1, invalid=None, invalid_any=16), nbytes=0) == E_INVALID and b"workspace too small" in err()
    assert call(_args(policy=2, invalid=None, weights=None, invalid_wsum=16), nbytes=0) == E_INVALID and b"workspace too small" in err()


def _level(n=1, pc=2, h=8, w=8, nv=2, K=3):
    level = dict(rgb=torch.rand(n, pc, h, w, nv, 3), depth=torch.rand(n, pc, h, w) + 1, weights=torch.rand(n, pc, h, w, K),
                 invalid=torch.zeros(n, pc, h, w, K, nv), rgb_samps=torch.rand(n, pc, h, w, K, nv, 3))
    return level, torch.rand(n, pc, h, w, 3)


def test_no_cpu_fallback():
    level, gt = _level()
    for conf in (dict(invalid_policy="weight_guided"), dict(invalid_policy="none"), dict(invalid_policy="weight_guided_diverse", native_pixel_loss=True)):
        crit = bts.ReconstructionLoss(dict(BASE, lambda_edge_aware_smoothness=0.01, **conf, **KEY))
        with pytest.raises(bts.BtsNativeError):
            crit(dict(coarse=[level], fine=[dict(level)], rgb_gt=gt))
    with pytest.raises(bts.BtsNativeError):
        bts.native.photometric_loss_median(level["rgb"].reshape(-1, 6), None, None, None, gt.reshape(-1, 3), 1, 8, 8, "none", False)


def test_the_native_wrapper_refuses_what_the_entry_cannot_take():
    level, gt = _level()
    rgb, g = level["rgb"].reshape(-1, 6), gt.reshape(-1, 3)
    with pytest.raises(bts.BtsNativeError, match="weight_guided_diverse"):
        bts.native.photometric_loss_median(rgb, None, None, None, g, 1, 8, 8, "weight_guided_diverse", False)
    with pytest.raises(bts.BtsNativeError, match="3 samples of whole 8x8 patches"):
        bts.native.photometric_loss_median(rgb, None, None, None, g, 3, 8, 8, "none", False)


@pytest.fixture(scope="module")
def golden():
    return np.load(MO.GOLDEN)


def _restated(z, layout, cname, mutant=None, grad=True):
    level, gt, bound = MO.load_inputs(z, layout)
    level["rgb"].requires_grad_(grad), level["depth"].requires_grad_(grad)
    loss, o = MO.reconstruction_loss(level, gt, MO.config_of(cname), bound=bound if MO.automasked(cname) else None, mutant=mutant)
    g = torch.autograd.grad(loss, [level["rgb"], level["depth"]]) if grad else (None, None)
    return loss.detach(), o, g[0], g[1]


@pytest.mark.parametrize("cname", list(MO.CONFIGS))
@pytest.mark.parametrize("layout", list(MO.LAYOUTS))
def test_the_restatement_reproduces_the_reference(golden, layout, cname):
    z = golden
    n, pc, h, w, nv, K = MO.LAYOUTS[layout]
    loss, o, g_rgb, g_depth = _restated(z, layout, cname)
    assert g_rgb.shape == (n, pc, h, w, nv, 3)
    key = f"{layout}_{cname}"
    want = dict(zip(MO.DICT_KEYS, z[f"{key}_loss_dict"].tolist()))
    assert abs(loss.item() - z[f"{key}_loss"].item()) <= 1e-6
    assert abs(2 * o["loss_rgb"].item() - want["loss_rgb_coarse"] - want["loss_rgb_fine"]) <= 2e-6
    assert abs(o["loss_eas"].item() - want["loss_eas"]) <= 1e-6 * max(1.0, abs(want["loss_eas"]))
    assert abs(o["loss_invalid_ratio"].item() - want["loss_invalid_ratio"]) <= 1e-6
    for got, ref in ((g_rgb, z[f"{key}_g_rgb"]), (g_depth, z[f"{key}_g_depth"])):
        ref = torch.from_numpy(ref)
        assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert torch.equal(o["thresholds"], torch.from_numpy(z[f"{key}_thresholds"])) and o["kept"] == int(z[f"{key}_kept"][0])
    D, rank = z[f"{layout}_D"].item(), (pc * h * w - 1) // 2
    assert 1e-6 < D < 2e-5
    assert (torch.from_numpy(z[f"{key}_thresholds64"]) - o["thresholds"].double()).abs().max().item() <= D
    # what makes the comparison with a kernel meaningful: nothing within 20 D above a threshold
    e, thr = o["e"].reshape(n, -1), o["thresholds"]
    for s in range(n):
        assert (e[s][e[s] > thr[s]].min() - thr[s]).item() >= 20 * D
    if layout == "p8":      # the <= tie: the value at sample 0's rank also sits one rank above it
        srt = e[0].sort().values
        assert srt[rank] == srt[rank + 1] == thr[0] and int((e[0] <= thr[0]).sum()) == rank + 2
    policy = MO.CONFIGS[cname]["invalid_policy"]
    assert (thr[-1].item() == 0.0) == (layout == "odd" and policy != "none")          # more than half invalid: threshold 0


MUTANT_CASES = [("upper_median", "ragged", "none"), ("upper_median", "p8", "wg"), ("strict_less", "p8", "wg"), ("strict_less", "odd", "strict_lean"),
                ("mask_at_receiver", "ragged", "wg"), ("mask_at_receiver", "frame", "diverse"), ("rank_before_keep", "odd", "wg"),
                ("rank_before_keep", "odd", "diverse"), ("rank_before_bound", "ragged", "wg_automask"), ("rank_before_bound", "frame", "wg_automask")]


@pytest.mark.parametrize("mutant,layout,cname", MUTANT_CASES)
def test_each_mutant_moves_the_golden_beyond_the_bars(golden, mutant, layout, cname):
    z, key = golden, f"{layout}_{cname}"
    loss, o, g_rgb, _ = _restated(z, layout, cname, mutant=mutant)
    ref = torch.from_numpy(z[f"{key}_g_rgb"])
    d_loss, d_kept = abs(loss.item() - z[f"{key}_loss"].item()), o["kept"] - int(z[f"{key}_kept"][0])
    d_grad = (g_rgb - ref).abs().max().item() / ref.abs().max().item()
    print(mutant, key, "loss", d_loss, "kept", d_kept, "gradient", d_grad)
    assert d_loss > 1e-5 or d_kept != 0 or d_grad > 1e-4
    if mutant == "mask_at_receiver":
        assert d_loss <= 1e-6 and d_kept == 0 and d_grad > 1e-4       # only the gradient tells


def test_the_golden_is_small(golden):
    assert os.path.getsize(MO.GOLDEN) < 1_000_000
    assert set(MO.MUTANTS) == {m for m, _, _ in MUTANT_CASES}
