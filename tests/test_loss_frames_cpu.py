"""CPU: the C ABI of the tiled photometric loss (bts_photometric_loss_tiled: patches of any size, whole frames) -- exports, workspace
size, argument errors as codes with messages before anything is launched -- and the CPU oracle restatement of the reference's loss
against tests/golden/loss_frames.npz (the REAL reference's ReconstructionLoss on a 16 x 16 patch layout and a 40 x 72 frame layout,
tests/golden/gen_golden_loss_frames.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import _lib
from behindthescenes_amd.build import build_library
from oracle import bts_loss as OL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_frames.npz")
E_INVALID = -1       # what the layout check of bts_photometric_loss returns


@pytest.fixture(scope="module")
def lib():
    build_library()          # hipcc cross-compiles for gfx950 without a GPU
    return _lib.load()


def _args(n_patches=2, ph=16, pw=16, nv=3, K=5, policy=2, eas=1, **ptrs):
    """A BtsLossArgs whose pointers are non-NULL dummies: the calls below must fail before anything is read or launched."""
    d = dict(rgb=16, depth=16, weights=16, invalid=16, rgb_gt=16, parts=16, g_rgb=None, g_depth=None, invalid_wsum=None, invalid_any=None)
    d.update(ptrs)
    return _lib.BtsLossArgs(n_patches=n_patches, patch_h=ph, patch_w=pw, nv=nv, K=K, invalid_policy=policy, edge_aware_smoothness=eas,
                            scale_rgb=1.0, scale_eas=1.0, **d)


def test_symbols_export_and_the_abi_version_stays(lib):
    for name in ("bts_photometric_loss_tiled", "bts_photometric_loss_tiled_workspace"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.bts_abi_version() == _lib.ABI_VERSION == 9


def test_workspace_size_is_positive_and_monotone(lib):
    ws = lib.bts_photometric_loss_tiled_workspace
    assert ws(1, 1, 1, 1) > 0 and ws(1, 192, 640, 1) > 0
    for a, b in (((1, 16, 16, 3), (2, 16, 16, 3)), ((4, 16, 16, 3), (4, 17, 16, 3)), ((4, 16, 16, 3), (4, 16, 17, 3)),
                 ((1, 40, 72, 3), (1, 192, 640, 3)), ((2, 9, 8, 1), (2, 9, 8, 2)), ((2, 9, 8, 2), (2, 9, 8, 8)),
                 ((1, 1, 70, 2), (1, 1, 71, 2)), ((255, 16, 16, 4), (256, 16, 16, 4))):
        assert ws(*a) <= ws(*b), (a, b)


def test_argument_errors_are_codes_with_messages(lib):
    need = lib.bts_photometric_loss_tiled_workspace(2, 16, 16, 3)
    a = _args(rgb=None)
    assert lib.bts_photometric_loss_tiled(C.byref(a), 16, need, None) == E_INVALID
    assert len(lib.bts_last_error()) > 0 and b"bts_photometric_loss_tiled" in lib.bts_last_error()
    a = _args()
    assert lib.bts_photometric_loss_tiled(C.byref(a), 16, need - 1, None) == E_INVALID
    assert b"workspace" in lib.bts_last_error()
    assert lib.bts_photometric_loss_tiled(C.byref(a), None, need, None) == E_INVALID
    a = _args(policy=2, weights=None, invalid_wsum=None)
    assert lib.bts_photometric_loss_tiled(C.byref(a), 16, need, None) == E_INVALID
    assert b"invalid_policy" in lib.bts_last_error()
    a = _args(n_patches=1 << 20, ph=64, pw=64)                      # 2^32 rays
    assert lib.bts_photometric_loss_tiled(C.byref(a), 16, 1 << 40, None) == E_INVALID
    assert b"rays" in lib.bts_last_error()


def test_the_wave_kernel_still_rejects_more_than_64_pixels(lib):
    a = _args(n_patches=1, ph=9, pw=8)
    assert lib.bts_photometric_loss(C.byref(a), None) == E_INVALID
    assert len(lib.bts_last_error()) > 0


@pytest.mark.parametrize("name", ["patch16", "frame"])
def test_oracle_reproduces_the_reference_on_large_patches(name):
    z = np.load(GOLDEN)
    t = {k: torch.from_numpy(z[f"{name}_{k}"]) for k in ("rgb", "depth", "weights", "invalid", "rgb_gt", "loss", "loss_dict", "g_rgb", "g_depth")}
    rgb, depth = t["rgb"].clone().requires_grad_(True), t["depth"].clone().requires_grad_(True)
    loss, parts = OL.reconstruction_loss(dict(rgb=rgb, depth=depth, weights=t["weights"], invalid=t["invalid"].float()), t["rgb_gt"],
                                         invalid_policy="weight_guided", lambda_eas=0.01)
    g_rgb, g_depth = torch.autograd.grad(loss, [rgb, depth])
    assert abs(loss.item() - t["loss"].item()) <= 1e-6
    want = dict(zip(["loss_rgb_coarse", "loss_rgb_fine", "loss_eas", "loss_invalid_ratio", "loss"], t["loss_dict"].tolist()))
    assert abs(parts["loss_eas"].item() - want["loss_eas"]) <= 1e-6 * max(1.0, abs(want["loss_eas"]))
    assert abs(parts["loss_invalid_ratio"].item() - want["loss_invalid_ratio"]) <= 1e-6
    for got, ref in ((g_rgb, t["g_rgb"]), (g_depth, t["g_depth"])):
        assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_no_cpu_fallback_for_large_patches():
    n, pc, h, w, nv, K = 1, 2, 16, 16, 2, 3
    level = dict(rgb=torch.rand(n, pc, h, w, nv, 3), depth=torch.rand(n, pc, h, w) + 1, weights=torch.rand(n, pc, h, w, K),
                 invalid=torch.zeros(n, pc, h, w, K, nv))
    crit = bts.ReconstructionLoss({"criterion": "l1+ssim", "invalid_policy": "weight_guided", "lambda_edge_aware_smoothness": 0.01})
    with pytest.raises(bts.BtsNativeError):
        crit(dict(coarse=[level], fine=[dict(level)], rgb_gt=torch.rand(n, pc, h, w, 3)))
