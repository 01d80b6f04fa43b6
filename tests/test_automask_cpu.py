"""CPU (no GPU, no kernel launches): auto-masking -- what ReconstructionLoss(conf, use_automasking=True) constructs with the opt-in
`native_automask: true` and what it still refuses, reconstruct()'s shapes with channels = 4, the C ABI of bts_automask_errors and the
three _automask loss entry points (exports, every BTS_E_INVALID path before anything is launched), the loud refusal of CPU tensors,
and the CPU restatement tests/_automask_oracle.py against tests/golden/automask.npz (the REAL reference's compute_errors_l1ssim inside
trainer.py:203-206 and its ReconstructionLoss(cfg, True): tests/golden/gen_golden_automask.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import _lib
from behindthescenes_amd.build import build_library
from tests import _automask_oracle as AO

E_INVALID = -1
KEY = {"native_automask": True}
PIXEL = {"native_pixel_loss": True}


@pytest.fixture(scope="module")
def lib():
    build_library()          # hipcc cross-compiles for gfx950 without a GPU
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(AO.GOLDEN)


# ---- construction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["none", "strict", "weight_guided"])
def test_with_the_key_automasking_constructs_for_the_shipped_criterion(policy):
    crit = bts.ReconstructionLoss(dict(criterion="l1+ssim", invalid_policy=policy, **KEY), use_automasking=True)
    assert crit.use_automasking and crit.native_automask


@pytest.mark.parametrize("name", list(AO.CONFIGS))
def test_the_goldens_configurations_construct(name):
    crit = bts.ReconstructionLoss(dict(AO.config_of(name), **KEY, **PIXEL), use_automasking=True)
    assert crit.use_automasking and crit.get_loss_metric_names() == ["loss", "loss_rgb_coarse", "loss_rgb_fine", "loss_ray_entropy", "loss_depth_reg"]


@pytest.mark.parametrize("crit", ["l1", "l2"])
@pytest.mark.parametrize("policy", ["none", "strict", "weight_guided", "weight_guided_diverse"])
@pytest.mark.parametrize("median", [False, True])
def test_with_both_keys_every_pixel_criterion_constructs(crit, policy, median):
    bts.ReconstructionLoss(dict(criterion=crit, invalid_policy=policy, median_thresholding=median, **KEY, **PIXEL), use_automasking=True)


def test_without_the_key_it_still_raises_and_the_message_names_the_key():
    for conf in ({"criterion": "l1+ssim"}, {"criterion": "l2", **PIXEL}, {"criterion": "l1+ssim", "native_automask": False}):
        with pytest.raises(NotImplementedError, match="use_automasking=True") as e:
            bts.ReconstructionLoss(conf, use_automasking=True)
        assert "native_automask: true" in str(e.value)


def test_what_the_key_does_not_open():
    with pytest.raises(NotImplementedError, match=r"'l1\+ssim' with median_thresholding=True"):
        bts.ReconstructionLoss(dict(criterion="l1+ssim", median_thresholding=True, **KEY, **PIXEL), use_automasking=True)
    for conf in (dict(criterion="l2"), dict(criterion="l1", median_thresholding=True), dict(criterion="l1+ssim", invalid_policy="weight_guided_diverse")):
        with pytest.raises(NotImplementedError, match="native_pixel_loss: true"):      # the pixel criteria keep their own opt-in
            bts.ReconstructionLoss(dict(conf, **KEY), use_automasking=True)
    crit = bts.ReconstructionLoss(dict(criterion="l1+ssim", **KEY))                   # the key alone changes nothing
    assert not crit.use_automasking


def test_a_three_channel_ground_truth_is_refused_with_a_message():
    crit = bts.ReconstructionLoss(dict(criterion="l1+ssim", **KEY), use_automasking=True)
    level = dict(rgb=torch.rand(1, 1, 8, 8, 2, 3), depth=torch.ones(1, 1, 8, 8), weights=torch.rand(1, 1, 8, 8, 4), invalid=torch.zeros(1, 1, 8, 8, 4, 2))
    with pytest.raises(ValueError, match="fourth channel"):
        crit(dict(coarse=[level], fine=[dict(level)], rgb_gt=torch.rand(1, 1, 8, 8, 3)))
    with pytest.raises(bts.BtsNativeError):       # CPU tensors: no fallback
        crit(dict(coarse=[level], fine=[dict(level)], rgb_gt=torch.rand(1, 1, 8, 8, 4)))


# ---- samplers -------------------------------------------------------------------------------------------------------
def _render_dict(n, rays, nv, K, lean):
    part = dict(rgb=torch.rand(n, rays, nv * 3), depth=torch.rand(n, rays))
    if lean:
        part.update(invalid_wsum=torch.zeros(n, rays, nv), invalid_any=torch.zeros(n, rays, nv))
    else:
        part.update(weights=torch.rand(n, rays, K), invalid=torch.zeros(n, rays, K, nv), alphas=torch.rand(n, rays, K), rgb_samps=torch.rand(n, rays, K, nv * 3))
    return dict(coarse=part, fine=dict(part), rgb_gt=torch.rand(n, rays, 4))


@pytest.mark.parametrize("lean", [False, True])
def test_reconstruct_with_four_channels_reshapes_the_render_with_three(lean):
    n, nv, K = 2, 3, 5
    smp = bts.PatchRaySampler(ray_batch_size=128, z_near=3, z_far=80, patch_size=8, channels=4)
    rd = smp.reconstruct(_render_dict(n, 128, nv, K, lean))
    assert rd["coarse"]["rgb"].shape == (n, 2, 8, 8, nv, 3) and rd["rgb_gt"].shape == (n, 2, 8, 8, 4)
    if not lean:
        assert rd["coarse"]["rgb_samps"].shape == (n, 2, 8, 8, K, nv, 3) and rd["coarse"]["invalid"].shape == (n, 2, 8, 8, K, nv)
    img = bts.ImageRaySampler(3, 80, height=6, width=10, channels=4)
    rd = img.reconstruct(_render_dict(n, 2 * 60, nv, K, lean))
    assert rd["fine"]["rgb"].shape == (n, 2, 6, 10, nv, 3) and rd["rgb_gt"].shape == (n, 2, 6, 10, 4)
    rnd = bts.RandomRaySampler(50, 3, 80, channels=4)
    rd = rnd.reconstruct(_render_dict(n, 50, nv, K, lean))
    assert rd["coarse"]["rgb"].shape == (n, 50, nv, 3) and rd["rgb_gt"].shape == (n, 50, 4)
    # three channels: as ever
    rd = bts.PatchRaySampler(128, 3, 80, 8).reconstruct(dict(_render_dict(n, 128, nv, K, lean), rgb_gt=torch.rand(n, 128, 3)))
    assert rd["coarse"]["rgb"].shape == (n, 2, 8, 8, nv, 3) and rd["rgb_gt"].shape == (n, 2, 8, 8, 3)


# ---- the Python surface ---------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused_and_the_counts_must_agree():
    x = torch.rand(1, 3, 3, 8, 8)
    with pytest.raises(bts.BtsNativeError):
        bts.automask_images(x, [0, 1])
    with pytest.raises(bts.BtsNativeError):
        bts.automask_errors(x, [0, 1], n_render=2)
    with pytest.raises(ValueError) as e:
        bts.automask_images(x, [0, 1], n_render=3)
    assert "2 loss frames" in str(e.value) and "len(ids_render) = 3" in str(e.value)
    for bad in ([], [3], [-1], list(range(3)) * 3):
        with pytest.raises(ValueError, match="ids_loss"):
            bts.automask_errors(x, bad)
    with pytest.raises(ValueError, match="processed frames"):
        bts.automask_errors(torch.rand(1, 3, 4, 8, 8), [0])
    assert bts.automask.automask_images is bts.automask_images and "automask_errors" in bts.__all__


def test_the_torch_composed_modes_refuse_a_four_channel_images_alt():
    from behindthescenes_amd import synthetic as S
    H, W = 16, 32
    net = bts.BTSNet(S.field_conf(64, 64, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), 64, num_views=2)
    scene = S.synthetic_scene(1, 3, H, W, 64, seed=1)
    alt = torch.rand(1, 3, 4, H, W)
    with pytest.raises(NotImplementedError, match="4-channel images_alt"):      # two encoder views: a torch-composed mode
        net.encode(scene["images"], scene["projs"], scene["poses"], ids_encoder=[0, 1], ids_render=[1, 2], images_alt=alt)


# ---- the C ABI ------------------------------------------------------------------------------------------------------
NEW = ("bts_automask_errors", "bts_photometric_loss_automask", "bts_photometric_loss_tiled_automask_workspace",
       "bts_photometric_loss_tiled_automask", "bts_pixel_loss_automask")


def test_symbols_export_and_the_abi_version_stays(lib):
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert lib.bts_abi_version() == _lib.ABI_VERSION == 9
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bts_render.h")).read()
    for name in NEW:
        assert name + "(" in header, name
    base, thr = lib.bts_photometric_loss_tiled_workspace, lib.bts_photometric_loss_tiled_automask_workspace
    assert thr(4, 16, 16, 2) > base(4, 16, 16, 2) > 0 and thr(0, 16, 16, 2) >= 0 and thr(4, 0, 16, 2) == 0


def _loss_args(**over):
    d = dict(rgb=16, depth=16, weights=16, invalid=16, rgb_gt=16, parts=16, g_rgb=None, g_depth=None, n_patches=2, patch_h=8, patch_w=8, nv=2, K=4,
             invalid_policy=2, edge_aware_smoothness=1, scale_rgb=1.0, scale_eas=1.0, invalid_wsum=None, invalid_any=None)
    d.update(over)
    return _lib.BtsLossArgs(**d)


def _pixel_args(**over):
    d = dict(rgb=16, rgb_gt=16, depth=16, weights=16, invalid=16, invalid_wsum=None, invalid_any=None, rgb_samps=16, out=16, thresholds=None,
             kept=None, g_rgb=None, g_depth=None, B=384, n=2, patch_h=8, patch_w=8, nv=3, K=5, criterion=2, invalid_policy=1,
             median_thresholding=1, edge_aware_smoothness=1, scale_rgb=1.0, scale_eas=1.0)
    d.update(over)
    return _lib.BtsPixelLossArgs(**d)


def test_a_null_threshold_and_every_base_check_fail_before_any_launch(lib):
    """(the pointers are non-NULL dummies: a call that got as far as reading or launching anything would fault)"""
    err = lambda: lib.bts_last_error()
    wave = lambda a, t=16: lib.bts_photometric_loss_automask(C.byref(a) if a is not None else None, t, None)
    need = lib.bts_photometric_loss_tiled_automask_workspace(2, 16, 16, 2)
    tiled = lambda a, t=16, ws=16, nb=need: lib.bts_photometric_loss_tiled_automask(C.byref(a) if a is not None else None, t, ws, nb, None)
    pneed = lib.bts_pixel_loss_workspace(384, 2, 8, 8)
    pixel = lambda a, t=16, ws=16, nb=pneed: lib.bts_pixel_loss_automask(C.byref(a) if a is not None else None, t, ws, nb, None)
    big = dict(patch_h=16, patch_w=16)
    # thresh == NULL
    assert wave(_loss_args(), None) == E_INVALID and b"bts_photometric_loss_automask: thresh is NULL" in err()
    assert tiled(_loss_args(**big), None) == E_INVALID and b"bts_photometric_loss_tiled_automask: thresh is NULL" in err()
    assert pixel(_pixel_args(), None) == E_INVALID and b"bts_pixel_loss_automask: thresh is NULL" in err()
    # the base entry points' checks, under the new names
    assert wave(None) == E_INVALID and b"bts_photometric_loss_automask" in err()
    for over in (dict(rgb=None), dict(rgb_gt=None), dict(parts=None), dict(n_patches=-1), dict(patch_h=0), dict(patch_h=9), dict(nv=0),
                 dict(invalid_policy=3), dict(invalid_policy=1, invalid=None), dict(weights=None), dict(depth=None)):
        assert wave(_loss_args(**over)) == E_INVALID and b"bts_photometric_loss_automask" in err(), over
    assert tiled(None) == E_INVALID and b"bts_photometric_loss_tiled_automask" in err()
    for over in (dict(rgb=None), dict(rgb_gt=None), dict(parts=None), dict(patch_w=0), dict(nv=0), dict(invalid_policy=-1), dict(depth=None)):
        assert tiled(_loss_args(**dict(big, **over))) == E_INVALID and b"bts_photometric_loss_tiled_automask" in err(), over
    assert tiled(_loss_args(**big, weights=None)) == E_INVALID and b"invalid_policy 2 needs" in err()
    assert tiled(_loss_args(n_patches=1 << 23, **big)) == E_INVALID and b"2^31 - 1 rays" in err()
    assert tiled(_loss_args(**big), nb=need - 1) == E_INVALID and b"bts_photometric_loss_tiled_automask_workspace" in err()
    assert tiled(_loss_args(**big), ws=None) == E_INVALID and b"workspace too small" in err()
    # (the base entry's smaller workspace is too small for the form with the bound)
    assert tiled(_loss_args(**big), nb=lib.bts_photometric_loss_tiled_workspace(2, 16, 16, 2)) == E_INVALID and b"workspace too small" in err()
    assert pixel(None) == E_INVALID and b"bts_pixel_loss_automask" in err() and b"NULL required pointer" in err()
    for over, msg in ((dict(rgb=None), b"NULL required pointer"), (dict(B=0), b"non-positive size"), (dict(B=385), b"not a multiple"),
                      (dict(criterion=3), b"unknown criterion"), (dict(invalid_policy=4), b"unknown invalid_policy"),
                      (dict(invalid_policy=3, rgb_samps=None), b"weight_guided_diverse needs"), (dict(invalid=None), b"invalid_policy 1 needs")):
        assert pixel(_pixel_args(**over)) == E_INVALID and msg in err() and b"bts_pixel_loss_automask" in err(), over
    assert pixel(_pixel_args(), nb=pneed - 1) == E_INVALID and b"workspace too small" in err()
    # the base entry points answer under their own names, as before
    assert lib.bts_photometric_loss(C.byref(_loss_args(rgb=None)), None) == E_INVALID and b"bts_photometric_loss:" in err()
    assert lib.bts_pixel_loss(C.byref(_pixel_args(B=385)), 16, pneed, None) == E_INVALID and b"bts_pixel_loss:" in err()


def test_the_map_entry_checks_its_arguments_before_any_launch(lib):
    err = lambda: lib.bts_last_error()
    ids = lambda *v: (C.c_int32 * max(len(v), 1))(*v)

    def call(images=16, n=1, v=4, H=8, W=8, idl=ids(0, 2), L=2, errors=16, images4=16):
        return lib.bts_automask_errors(images, n, v, H, W, idl, L, 0.5, errors, images4, None)
    assert call(images=None) == E_INVALID and b"bts_automask_errors: NULL images or ids_loss" in err()
    assert call(idl=None) == E_INVALID and b"NULL images or ids_loss" in err()
    assert call(errors=None, images4=None) == E_INVALID and b"both outputs" in err()
    for k in ("n", "v", "H", "W"):
        assert call(**{k: 0}) == E_INVALID and b"non-positive size" in err(), k
    for L in (0, -1, _lib.BTS_MAX_VIEWS + 1):
        assert call(idl=ids(*([0] * 9)), L=L) == E_INVALID and b"outside [1, BTS_MAX_VIEWS" in err(), L
    for bad in ((0, 4), (-1, 0), (2, 0, 7)):
        assert call(idl=ids(*bad), L=len(bad)) == E_INVALID and b"is outside [0, v = 4)" in err(), bad
    assert call(n=1 << 30, H=64, W=64) == E_INVALID and b"2^31 - 1 tiles" in err()


# ---- the restatement against the real reference ---------------------------------------------------------------------
@pytest.mark.parametrize("case", list(AO.MAP_CASES))
def test_the_maps_restatement_reproduces_the_reference(golden, case):
    n, v, H, W, ids = AO.MAP_CASES[case]
    x = AO.map_frames(golden, case)
    assert x.shape == (n, v, 3, H, W) and golden[f"map_{case}_ids"].tolist() == ids
    m32, m64, dist = torch.from_numpy(golden[f"map_{case}_ref32"]), torch.from_numpy(golden[f"map_{case}_ref64"]), golden[f"map_{case}_dist"].item()
    assert (AO.error_map(x, ids)[:, :, 0] - m32).abs().max().item() <= 1e-6
    assert (AO.error_map(x.double(), ids)[:, :, 0] - m64).abs().max().item() <= 1e-12
    assert 0 < dist < 1e-5 and abs((m32.double() - m64).abs().max().item() - dist) <= 1e-12
    four = AO.images4(x, ids)
    assert four.shape == (n, v, 4, H, W) and torch.equal(four[:, :, :3], x)
    band = slice(H // 3, H // 3 + max(H // 6, 1))      # identical in all views: only the zero padding at the frame's sides makes an error
    assert m64[:, :, band, 1:-1][:, :, 1:-1].abs().max().item() <= 1e-9 if H >= 18 else True
    assert m64.max().item() > 0.05


def test_each_map_mutant_leaves_the_bar(golden):
    for m in AO.MAP_MUTANTS:
        moved = []
        for case, (_, _, _, _, ids) in AO.MAP_CASES.items():
            d = (AO.error_map(AO.map_frames(golden, case), ids, mutant=m)[:, :, 0].double() - torch.from_numpy(golden[f"map_{case}_ref64"])).abs().max().item()
            moved.append(d > 2 * golden[f"map_{case}_dist"].item())
        assert any(moved), m


@pytest.mark.parametrize("cname", list(AO.CONFIGS))
@pytest.mark.parametrize("layout", list(AO.LAYOUTS))
def test_the_loss_restatement_reproduces_the_reference(golden, layout, cname):
    z = golden
    level, gt = AO.load_inputs(z, layout)
    n, pc, h, w, nv, K = AO.LAYOUTS[layout]
    assert level["rgb"].shape == (n, pc, h, w, nv, 3) and level["invalid"].shape == (n, pc, h, w, K, nv)
    thresh = AO.load_thresh(z, layout, cname)
    level["rgb"].requires_grad_(True), level["depth"].requires_grad_(True)
    loss, o = AO.reconstruction_loss(level, torch.cat((gt, thresh.unsqueeze(-1)), -1), AO.config_of(cname))
    g_rgb, g_depth = torch.autograd.grad(loss, [level["rgb"], level["depth"]])
    key = f"am_{layout}_{cname}"
    want = dict(zip(AO.DICT_KEYS, z[f"{key}_loss_dict"].tolist()))
    assert abs(loss.item() - z[f"{key}_loss"].item()) <= 1e-6
    assert abs(2 * o["loss_rgb"].item() - want["loss_rgb_coarse"] - want["loss_rgb_fine"]) <= 2e-6
    assert abs(o["loss_eas"].item() - want["loss_eas"]) <= 1e-6 * max(1.0, abs(want["loss_eas"]))
    assert abs(o["loss_invalid_ratio"].item() - want["loss_invalid_ratio"]) <= 1e-6
    for got, ref in ((g_rgb, z[f"{key}_g_rgb"]), (g_depth, z[f"{key}_g_depth"])):
        ref = torch.from_numpy(ref)
        assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert 0.2 <= o["bound"] <= 0.8                       # the bound neither always wins nor always loses
    # no compared value within 1e-4 of its bound outside the constructed block, where l1 / l2 tie exactly
    e0 = AO.errors_before_bound(level, gt, AO.config_of(cname)).detach()
    block = torch.from_numpy(z[f"am_{layout}_tie_block"])
    gap = (e0 - thresh.unsqueeze(-1)).abs()
    if AO.crit_key(cname) == "ssim":
        assert (gap > 1e-4).all()
    else:
        assert (gap[~block] > 1e-4).all() and (gap[block] == 0).all() and block.any()
        assert (thresh[block] == AO.TIE[AO.crit_key(cname)]).all()


def test_the_golden_is_small_and_a_tie_takes_half_the_gradient(golden):
    assert os.path.getsize(AO.GOLDEN) < 1_000_000
    level, gt = AO.load_inputs(golden, "p16")
    thresh = AO.load_thresh(golden, "p16", "l2")
    block = torch.from_numpy(golden["am_p16_tie_block"])
    g = torch.from_numpy(golden["am_p16_l2_g_rgb"])          # (n, pc, h, w, nv, 3)
    level["rgb"].requires_grad_(True)
    cfg = dict(criterion="l2", invalid_policy="none")
    loss, _ = AO.reconstruction_loss(level, torch.cat((gt, torch.full_like(thresh, float("inf")).unsqueeze(-1)), -1), cfg)
    free, = torch.autograd.grad(loss, [level["rgb"]])        # no bound: the full gradient
    keep = AO.PO.invalid_rays(level, "strict").squeeze(-1) == 0
    sel = block & keep
    assert sel.any() and torch.allclose(g[sel], 0.5 * free[sel], rtol=1e-6, atol=0) and free[sel].abs().max() > 0
