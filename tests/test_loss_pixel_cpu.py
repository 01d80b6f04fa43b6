"""CPU (no GPU, no kernel launches): the opt-in `native_pixel_loss: true` of ReconstructionLoss -- what constructs with the key and what
still refuses, the C ABI of bts_pixel_loss / bts_loss_diverse_flags (exports, struct layout against gcc, every BTS_E_INVALID path with
its message before anything is launched), the lean-dict KeyError of weight_guided_diverse, FusedTrainStep's answer to an opted-in
criterion, and the CPU restatement tests/_loss_pixel_oracle.py against tests/golden/loss_pixel.npz (the REAL reference's
ReconstructionLoss: tests/golden/gen_golden_loss_pixel.py)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import _lib
from behindthescenes_amd.build import build_library
from tests import _loss_pixel_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
KEY = {"native_pixel_loss": True}


@pytest.fixture(scope="module")
def lib():
    build_library()          # hipcc cross-compiles for gfx950 without a GPU
    return _lib.load()


@pytest.mark.parametrize("name", list(PO.CONFIGS))
def test_the_listed_configurations_construct_with_the_key(name):
    crit = bts.ReconstructionLoss(dict(PO.config_of(name), **KEY))
    assert crit.native_pixel_loss and crit.criterion_str == PO.CONFIGS[name].get("criterion", "l2")
    assert crit.get_loss_metric_names() == ["loss", "loss_rgb_coarse", "loss_rgb_fine", "loss_ray_entropy", "loss_depth_reg"]


@pytest.mark.parametrize("crit", ["l1", "l2"])
@pytest.mark.parametrize("policy", ["none", "strict", "weight_guided", "weight_guided_diverse"])
@pytest.mark.parametrize("median", [False, True])
def test_every_pixel_criterion_policy_and_median_constructs(crit, policy, median):
    bts.ReconstructionLoss(dict(criterion=crit, invalid_policy=policy, median_thresholding=median, **KEY))


def test_without_the_key_construction_still_raises_and_names_the_key():
    for conf in ({"criterion": "l2"}, {"criterion": "l1"}, {}, {"criterion": "l1", "median_thresholding": True},
                 {"criterion": "l1+ssim", "invalid_policy": "weight_guided_diverse"}, {"criterion": "l2", "native_pixel_loss": False}):
        with pytest.raises(NotImplementedError, match="native_pixel_loss: true"):
            bts.ReconstructionLoss(conf)


def test_with_the_key_ssim_median_and_automasking_still_raise_and_name_the_combination():
    with pytest.raises(NotImplementedError, match=r"'l1\+ssim' with median_thresholding=True"):
        bts.ReconstructionLoss(dict(criterion="l1+ssim", median_thresholding=True, **KEY))
    for conf in ({"criterion": "l1+ssim"}, {"criterion": "l2"}):
        with pytest.raises(NotImplementedError, match="use_automasking=True"):
            bts.ReconstructionLoss(dict(conf, **KEY), use_automasking=True)
    bts.ReconstructionLoss(dict(criterion="l1+ssim", **KEY))         # the key alone changes nothing for the shipped criterion


def test_the_new_struct_matches_the_c_layout():
    fields = [f[0] for f in _lib.BtsPixelLossArgs._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bts_render.h"\nint main(void) {\n  printf("%zu", sizeof(BtsPixelLossArgs));\n' + \
        "".join(f'  printf(" %zu", offsetof(BtsPixelLossArgs, {f}));\n' for f in fields) + '  printf(" %d", BTS_ABI_VERSION);\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.BtsPixelLossArgs) == 160
    assert out[1:-1] == [getattr(_lib.BtsPixelLossArgs, f).offset for f in fields]
    assert (_lib.BtsPixelLossArgs.B.offset, _lib.BtsPixelLossArgs.scale_rgb.offset) == (104, 152)
    assert out[-1] == _lib.ABI_VERSION == 9


def test_symbols_export_and_the_abi_version_stays(lib):
    for name in ("bts_pixel_loss", "bts_pixel_loss_workspace", "bts_loss_diverse_flags"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.bts_abi_version() == _lib.ABI_VERSION == 9
    assert bts.native.pixel_loss and bts.native.loss_diverse_flags


def test_workspace_size_is_positive_and_monotone(lib):
    ws = lib.bts_pixel_loss_workspace
    assert ws(64, 1, 8, 8) > 0 and ws(192 * 640, 1, 192, 640) > 0
    assert ws(0, 1, 8, 8) == 0 and ws(64, 0, 8, 8) == 0
    for a, b in (((64, 1, 8, 8), (128, 1, 8, 8)), ((128, 1, 8, 8), (128, 2, 8, 8)), ((2880, 1, 40, 72), (5760, 1, 40, 72)),
                 ((16 * 4096, 16, 8, 8), (32 * 4096, 16, 8, 8))):
        assert ws(*a) <= ws(*b), (a, b)


def _args(B=384, n=2, ph=8, pw=8, nv=3, K=5, crit=2, policy=1, median=1, eas=1, **ptrs):
    """A BtsPixelLossArgs whose pointers are non-NULL dummies: the calls below must fail before anything is read or launched."""
    d = dict(rgb=16, rgb_gt=16, depth=16, weights=16, invalid=16, invalid_wsum=None, invalid_any=None, rgb_samps=16, out=16, thresholds=None,
             kept=None, g_rgb=None, g_depth=None)
    d.update(ptrs)
    return _lib.BtsPixelLossArgs(B=B, n=n, patch_h=ph, patch_w=pw, nv=nv, K=K, criterion=crit, invalid_policy=policy, median_thresholding=median,
                                 edge_aware_smoothness=eas, scale_rgb=1.0, scale_eas=1.0, **d)


def test_argument_errors_are_codes_with_messages(lib):
    need = lib.bts_pixel_loss_workspace(384, 2, 8, 8)
    call = lambda a, ws=16, nbytes=need: lib.bts_pixel_loss(C.byref(a) if a is not None else None, ws, nbytes, None)
    err = lambda: lib.bts_last_error()
    assert call(None) == E_INVALID and b"bts_pixel_loss" in err() and b"NULL required pointer" in err()
    for k in ("rgb", "rgb_gt", "out", "depth"):
        assert call(_args(**{k: None})) == E_INVALID and b"NULL required pointer" in err(), k
    for k in ("B", "n", "ph", "pw", "nv"):
        assert call(_args(**{k: 0})) == E_INVALID and b"non-positive size" in err(), k
        assert call(_args(**{k: -3})) == E_INVALID and b"non-positive size" in err(), k
    assert call(_args(B=385)) == E_INVALID and b"not a multiple of n * patch_h * patch_w" in err()
    assert call(_args(B=64 * 3, n=2)) == E_INVALID and b"not a multiple" in err()            # whole patches, but not per sample
    assert call(_args(B=(1 << 29) + 64, n=1)) == E_INVALID and b"2^29" in err()
    for c in (0, 3, -1):
        assert call(_args(crit=c)) == E_INVALID and b"unknown criterion" in err(), c
    for p in (-1, 4):
        assert call(_args(policy=p)) == E_INVALID and b"unknown invalid_policy" in err(), p
    for k in ("rgb_samps", "weights", "invalid"):
        assert call(_args(policy=3, **{k: None})) == E_INVALID and b"weight_guided_diverse needs rgb_samps, weights and invalid" in err(), k
    assert call(_args(policy=3, K=0)) == E_INVALID and b"weight_guided_diverse" in err()
    assert call(_args(policy=1, invalid=None)) == E_INVALID and b"invalid_policy 1 needs" in err()
    assert call(_args(policy=2, weights=None)) == E_INVALID and b"invalid_policy 2 needs" in err()
    assert call(_args(), nbytes=need - 1) == E_INVALID and b"workspace too small" in err()
    assert call(_args(), ws=None) == E_INVALID and b"workspace too small" in err()
    # the flags' entry
    flags = lambda *a: lib.bts_loss_diverse_flags(*a, None)
    for bad in ((None, 16, 16, 8, 5, 3, 16), (16, None, 16, 8, 5, 3, 16), (16, 16, None, 8, 5, 3, 16), (16, 16, 16, 8, 5, 3, None),
                (16, 16, 16, 0, 5, 3, 16), (16, 16, 16, 8, 0, 3, 16), (16, 16, 16, 8, 5, 0, 16)):
        assert flags(*bad) == E_INVALID and b"bts_loss_diverse_flags" in err(), bad


def _level(n=1, pc=2, h=8, w=8, nv=2, K=3, lean=False):
    level = dict(rgb=torch.rand(n, pc, h, w, nv, 3), depth=torch.rand(n, pc, h, w) + 1)
    if lean:
        level.update(invalid_wsum=torch.zeros(n, pc, h, w, nv), invalid_any=torch.zeros(n, pc, h, w, nv))
    else:
        level.update(weights=torch.rand(n, pc, h, w, K), invalid=torch.zeros(n, pc, h, w, K, nv), rgb_samps=torch.rand(n, pc, h, w, K, nv, 3))
    return level, torch.rand(n, pc, h, w, 3)


@pytest.mark.parametrize("criterion", ["l2", "l1+ssim"])
@pytest.mark.parametrize("aliased_fine", [True, False])
def test_a_lean_render_dict_with_diverse_says_what_to_ask_the_renderer_for(criterion, aliased_fine):
    level, gt = _level(lean=True)
    crit = bts.ReconstructionLoss(dict(criterion=criterion, invalid_policy="weight_guided_diverse", **KEY))
    with pytest.raises(KeyError) as e:
        crit(dict(coarse=[level], fine=[dict(level) if aliased_fine else {}], rgb_gt=gt))
    assert "want_rgb_samps" in str(e.value) and "lean_training_outputs" in str(e.value) and "rgb_samps" in str(e.value)


def test_no_cpu_fallback_for_the_new_criteria():
    level, gt = _level()
    for conf in (dict(criterion="l2"), dict(criterion="l1", median_thresholding=True), dict(criterion="l1+ssim", invalid_policy="weight_guided_diverse")):
        crit = bts.ReconstructionLoss(dict(conf, lambda_edge_aware_smoothness=0.01, **KEY))
        with pytest.raises(bts.BtsNativeError):
            crit(dict(coarse=[level], fine=[dict(level)], rgb_gt=gt))


def test_the_fused_training_step_gives_a_reason_for_the_opted_in_criteria():
    from behindthescenes_amd.train_step import FusedTrainStep
    from behindthescenes_amd import synthetic as S
    H, W = 48, 64
    net = bts.BTSNet(S.field_conf(64, 64, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), 64, num_views=1)
    renderer = bts.NeRFRenderer.from_conf(dict(n_coarse=8, lindisp=True, hard_alpha_cap=True, lean_training_outputs=True)).train()
    sampler = bts.PatchRaySampler(ray_batch_size=128, z_near=3.0, z_far=80.0, patch_size=8)
    reasons = {}
    for name, conf in (("shipped", dict(criterion="l1+ssim", invalid_policy="weight_guided")), ("l2", dict(criterion="l2", **KEY)),
                       ("l1", dict(criterion="l1", invalid_policy="none", **KEY)),
                       ("median", dict(criterion="l1", median_thresholding=True, **KEY)),
                       ("diverse", dict(criterion="l1+ssim", invalid_policy="weight_guided_diverse", **KEY))):
        step = FusedTrainStep(renderer.bind_parallel(net).train(), sampler, bts.ReconstructionLoss(conf))
        reasons[name] = step.why_not(None, [0], [1], [0, 1])
    assert reasons["shipped"] is None, reasons
    assert "criterion l2" in reasons["l2"] and "criterion l1" in reasons["l1"] and "criterion l1" in reasons["median"]
    assert "weight_guided_diverse" in reasons["diverse"]
    # median thresholding is a reason of its own (no such loss can be constructed today: l1+ssim + median raises; the check stands guard)
    crit = bts.ReconstructionLoss(dict(criterion="l1+ssim", invalid_policy="weight_guided"))
    crit.median_thresholding = True
    assert "median_thresholding" in FusedTrainStep(renderer.bind_parallel(net).train(), sampler, crit).why_not(None, [0], [1], [0, 1])


@pytest.fixture(scope="module")
def golden():
    return np.load(PO.GOLDEN)


@pytest.mark.parametrize("cname", list(PO.CONFIGS))
@pytest.mark.parametrize("layout", list(PO.LAYOUTS))
def test_the_restatement_reproduces_the_reference(golden, layout, cname):
    z = golden
    level, gt = PO.load_inputs(z, layout)
    n, pc, h, w, nv, K = PO.LAYOUTS[layout]
    assert level["rgb"].shape == (n, pc, h, w, nv, 3) and level["rgb_samps"].shape == (n, pc, h, w, K, nv, 3)
    level["rgb"].requires_grad_(True), level["depth"].requires_grad_(True)
    loss, o = PO.reconstruction_loss(level, gt, PO.config_of(cname))
    g_rgb, g_depth = torch.autograd.grad(loss, [level["rgb"], level["depth"]])
    key = f"{layout}_{cname}"
    want = dict(zip(PO.DICT_KEYS, z[f"{key}_loss_dict"].tolist()))
    assert abs(loss.item() - z[f"{key}_loss"].item()) <= 1e-6
    assert abs(2 * o["loss_rgb"].item() - want["loss_rgb_coarse"] - want["loss_rgb_fine"]) <= 2e-6
    assert abs(o["loss_eas"].item() - want["loss_eas"]) <= 1e-6 * max(1.0, abs(want["loss_eas"]))
    assert abs(o["loss_invalid_ratio"].item() - want["loss_invalid_ratio"]) <= 1e-6
    for got, ref in ((g_rgb, z[f"{key}_g_rgb"]), (g_depth, z[f"{key}_g_depth"])):
        ref = torch.from_numpy(ref)
        assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    if PO.CONFIGS[cname].get("median_thresholding"):
        assert torch.equal(o["thresholds"], torch.from_numpy(z[f"{key}_thresholds"])) and o["kept"] == int(z[f"{key}_kept"][0])
        assert o["thresholds"][0].item() == (0.125 if cname.startswith("l1") else 0.015625)        # the plateau
        assert (o["thresholds"][-1].item() == 0.0) == (layout == "odd")                            # more than half invalid: threshold 0
    else:
        assert z[f"{key}_thresholds"].size == 0 and int(z[f"{key}_kept"][0]) == 3 * n * pc * h * w


def test_the_golden_is_small_and_its_mutants_differ(golden):
    assert os.path.getsize(PO.GOLDEN) < 1_000_000
    level, gt = PO.load_inputs(golden, "p8")
    base, _ = PO.reconstruction_loss(level, gt, PO.config_of("l1_median"))
    for m in ("upper_median", "strict_less", "min_after_mean"):
        other, _ = PO.reconstruction_loss(level, gt, PO.config_of("l1_median"), mutant=m)
        assert abs(other.item() - base.item()) > 1e-5, m
