"""CPU (no GPU, no kernel launches): the opt-in `native_regularisers: true` of ReconstructionLoss -- the key is accepted and stored,
without it the object never calls the new library entry, with it `_call` makes one call per scale with the coefficients the reference's
algebra asks for and assembles the nine-key dict from what comes back; the C ABI of bts_loss_regularisers (exports, struct layout
against gcc, every error path with its code and message before anything is launched, the workspace query); the lean-dict KeyError and
FusedTrainStep's refusal stay; and the CPU restatement tests/_loss_reg_oracle.py against tests/golden/loss_reg.npz (the REAL
reference's ReconstructionLoss: tests/golden/gen_golden_loss_reg.py)."""
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
from tests import _loss_reg_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2
KEY = {"native_regularisers": True}


@pytest.fixture(scope="module")
def lib():
    build_library()          # hipcc cross-compiles for gfx950 without a GPU
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(RO.GOLDEN)


def test_the_constructor_accepts_and_stores_the_key():
    base = dict(criterion="l1+ssim", invalid_policy="weight_guided")
    assert bts.ReconstructionLoss(dict(base, **RO.ALL, **KEY)).native_regularisers is True
    assert bts.ReconstructionLoss(dict(base, **RO.ALL)).native_regularisers is False
    assert bts.ReconstructionLoss(dict(base, native_regularisers=False)).native_regularisers is False
    for name in RO.CONFIGS:
        crit = bts.ReconstructionLoss(dict(RO.config_of(name), **KEY))
        assert crit.native_regularisers and crit.get_loss_metric_names() == ["loss", "loss_rgb_coarse", "loss_rgb_fine", "loss_ray_entropy",
                                                                             "loss_depth_reg"]
    with pytest.raises(ValueError):
        bts.ReconstructionLoss(dict(base, alpha_reg_reduction="batch", **KEY))


def _levels(S=2, n=1, pc=2, h=4, w=4, K=8, nv=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    masks = dict(weights=torch.rand(n, pc, h, w, K, generator=g), invalid=(torch.rand(n, pc, h, w, K, nv, generator=g) < 0.3).float())
    masks["weights"] = masks["weights"] / masks["weights"].sum(-1, keepdim=True)
    levels = [dict(masks, rgb=torch.rand(n, pc, h, w, nv, 3, generator=g), depth=torch.rand(n, pc, h, w, generator=g) + 2,
                   alphas=torch.rand(n, pc, h, w, K, generator=g) * 0.4) for _ in range(S)]
    return levels, torch.rand(n, pc, h, w, 3, generator=g)


def _stub_photometric(monkeypatch):
    """the photometric term needs the GPU: a stand-in that returns (0.25, 0, 0.125) per call"""
    monkeypatch.setattr(bts.ReconstructionLoss, "_photometric",
                        lambda self, level, level0, gt, eas: (torch.tensor(0.25), torch.tensor(0.0), torch.tensor(0.125)))


def test_without_the_key_the_native_entry_is_never_called(monkeypatch):
    """... and the result is the torch composition's: the restatement's regulariser terms on top of the stubbed photometric term"""
    calls = []
    monkeypatch.setattr(native, "loss_regularisers_packed", lambda *a, **k: calls.append(1))
    monkeypatch.setattr(native, "loss_regularisers", lambda *a, **k: calls.append(1))
    _stub_photometric(monkeypatch)
    levels, gt = _levels()
    cfg = dict(RO.ALL, criterion="l1+ssim", invalid_policy="strict", alpha_reg_reduction="slice")
    loss, d = bts.ReconstructionLoss(cfg)(dict(coarse=levels, fine=[dict(x) for x in levels], rgb_gt=gt))
    assert calls == []
    keep = 1 - torch.all(torch.any(levels[0]["invalid"] > .5, dim=-2), dim=-1).float()
    want, after = 0.0, 0.0
    for s, lv in enumerate(levels):
        _, share, aft = RO.regularisers(lv, keep, cfg, s, len(levels))
        want, after = want + 0.25 * 2 + share, after + aft
    want = want / len(levels) + after
    assert abs(loss.item() - want.item()) <= 1e-6 and abs(d["loss"] - want.item()) <= 1e-6
    assert list(d) == RO.DICT_KEYS and d["loss_ray_entropy"] > 0 and d["loss_depth_reg"] == d["loss_depth_smoothness"] > 0


def test_with_the_key_one_call_per_scale_carries_the_reference_coefficients(monkeypatch):
    """scale 0's call carries the entropy, undivided; the other coefficients are lambda / n_scales, the depth one the sum of both lambdas; a
    lambda of 0 contributes a coefficient of 0; keep() is not evaluated by torch (no torch.all / torch.any on this path)"""
    calls = []

    def fake(alphas, depth, **kw):
        calls.append((alphas, depth, kw))
        s = len(calls)
        out = torch.tensor([0.5 * s, 7.0, 0.25 * s, 0.125 * s, 3.0, 0.0625 * s])
        return out[:5], out[5:], None, None, out
    monkeypatch.setattr(native, "loss_regularisers_packed", fake)
    for name in ("all", "any"):
        monkeypatch.setattr(torch, name, lambda *a, **k: pytest.fail("keep() evaluated by torch"))
    _stub_photometric(monkeypatch)
    levels, gt = _levels(S=2)
    cfg = dict(RO.ALL, criterion="l1+ssim", invalid_policy="weight_guided", alpha_reg_reduction="slice", alpha_reg_fraction=0.2, **KEY)
    loss, d = bts.ReconstructionLoss(cfg)(dict(coarse=levels, fine=[dict(x) for x in levels], rgb_gt=gt))
    assert len(calls) == 2
    for s, (alphas, depth, kw) in enumerate(calls):
        assert alphas.shape == (32, 8) and depth.shape == (32,) and torch.equal(alphas, levels[s]["alphas"].reshape(32, 8))
        assert (kw["n"], kw["pc"], kw["ph"], kw["pw"], kw["policy"], kw["alpha_reg_reduction"], kw["alpha_reg_fraction"]) == \
            (1, 2, 4, 4, "weight_guided", "slice", 0.2)
        assert kw["coef"] == (0.05 / 2, 0.1 / 2, 0.02 if s == 0 else 0.0, (0.03 + 0.02) / 2)
        assert torch.equal(kw["weights"], levels[0]["weights"].reshape(32, 8)) and kw["invalid"].shape == (32, 8, 2)      # scale 0's
        assert kw["invalid_wsum"] is None and kw["invalid_any"] is None and kw["rgb_samps"] is None
    want = (0.25 * 2 + 0.25 * 2) / 2 + 0.0625 + 0.125
    assert abs(loss.item() - want) <= 1e-6 and list(d) == RO.DICT_KEYS
    assert (d["loss_alpha_reg"], d["loss_depth_reg"], d["loss_depth_smoothness"], d["loss_ray_entropy"]) == (1.5, 0.375, 0.375, 0.25)
    assert abs(d["loss"] - want) <= 1e-6 and d["loss_invalid_ratio"] == 0.125 and d["loss_rgb_coarse"] == 0.5
    # one lambda alone: the others' coefficients are 0 and, without an alpha term, alphas is not even handed over
    calls.clear()
    only = dict(criterion="l1+ssim", invalid_policy="none", lambda_depth_smoothness=0.5, **KEY)
    bts.ReconstructionLoss(only)(dict(coarse=levels[:1], fine=[{}], rgb_gt=gt))
    assert len(calls) == 1 and calls[0][0] is None and calls[0][2]["coef"] == (0.0, 0.0, 0.0, 0.5) and calls[0][2]["policy"] == "none"
    # ... and the depth term, which is never masked, asks for no keep flags under any policy
    calls.clear()
    bts.ReconstructionLoss(dict(only, invalid_policy="strict"))(dict(coarse=levels[:1], fine=[{}], rgb_gt=gt))
    assert calls[0][2]["policy"] == "none" and calls[0][2]["invalid"] is None and calls[0][2]["coef"] == (0.0, 0.0, 0.0, 0.5)
    # lean sums: invalid_wsum under weight_guided
    calls.clear()
    lean = [RO.lean_of(lv) for lv in levels[:1]]
    bts.ReconstructionLoss(dict(criterion="l1+ssim", invalid_policy="weight_guided", lambda_entropy=0.1, **KEY))(
        dict(coarse=lean, fine=[dict(lean[0])], rgb_gt=gt))
    kw = calls[0][2]
    assert kw["weights"] is None and kw["invalid"] is None and kw["invalid_wsum"].shape == (32, 2) and kw["coef"] == (0.0, 0.0, 0.1, 0.0)
    # the entropy alone over two scales: scale 0's call is the only one
    calls.clear()
    loss, d = bts.ReconstructionLoss(dict(criterion="l1+ssim", invalid_policy="none", lambda_entropy=0.1, **KEY))(
        dict(coarse=levels, fine=[{}, {}], rgb_gt=gt))
    assert len(calls) == 1 and calls[0][2]["coef"] == (0.0, 0.0, 0.1, 0.0) and d["loss_ray_entropy"] == 0.25
    assert abs(loss.item() - ((0.25 + 0.25) / 2 + 0.0625)) <= 1e-6


def test_no_regulariser_on_keeps_the_photometric_only_path(monkeypatch):
    seen = []
    monkeypatch.setattr(bts.ReconstructionLoss, "_call_photometric_only", lambda self, data: seen.append(1) or ("loss", "dict"))
    crit = bts.ReconstructionLoss(dict(criterion="l1+ssim", invalid_policy="weight_guided", **KEY))
    assert crit(dict(coarse=[{}], fine=[{}])) == ("loss", "dict") and seen == [1]


def test_a_lean_render_dict_keeps_raising_the_key_error_with_the_key():
    crit = bts.ReconstructionLoss({"criterion": "l1+ssim", "invalid_policy": "weight_guided", "lambda_alpha_reg": 0.1, **KEY})
    lean = dict(rgb=torch.zeros(1, 1, 8, 8, 1, 3), depth=torch.ones(1, 1, 8, 8), invalid_wsum=torch.zeros(1, 1, 8, 8, 1),
                invalid_any=torch.zeros(1, 1, 8, 8, 1))
    with pytest.raises(KeyError, match="want_alphas"):
        crit(dict(coarse=[lean], fine=[{}], rgb_gt=torch.zeros(1, 1, 8, 8, 3)))


def test_the_fused_training_step_keeps_naming_the_regularisers():
    from behindthescenes_amd import synthetic as S
    from behindthescenes_amd.train_step import FusedTrainStep
    H, W = 48, 64
    net = bts.BTSNet(S.field_conf(64, 64, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), 64, num_views=1)
    renderer = bts.NeRFRenderer.from_conf(dict(n_coarse=8, lindisp=True, hard_alpha_cap=True, lean_training_outputs=True)).train()
    sampler = bts.PatchRaySampler(ray_batch_size=128, z_near=3.0, z_far=80.0, patch_size=8)
    crit = bts.ReconstructionLoss(dict(criterion="l1+ssim", invalid_policy="weight_guided", lambda_depth_reg=0.1, **KEY))
    why = FusedTrainStep(renderer.bind_parallel(net).train(), sampler, crit).why_not(None, [0], [1], [0, 1])
    assert why == "an optional regulariser of the loss is on"


def test_no_cpu_fallback_and_a_one_pixel_wide_patch_is_a_value_error():
    a, d = torch.rand(16, 8), torch.rand(16)
    with pytest.raises(bts.BtsNativeError, match="GPU"):
        native.loss_regularisers(a, d, n=1, pc=1, ph=4, pw=4, policy="none", coef=(0.1, 0, 0, 0.1))
    for ph, pw in ((1, 16), (16, 1)):
        with pytest.raises(ValueError, match="at least 2 x 2"):
            native.loss_regularisers(a, d, n=1, pc=1, ph=ph, pw=pw, policy="none", coef=(0, 0, 0, 0.1))
    with pytest.raises(bts.BtsNativeError, match="alpha_reg_reduction"):
        native.loss_regularisers(a, d, n=1, pc=1, ph=4, pw=4, policy="none", coef=(0.1, 0, 0, 0), alpha_reg_reduction="batch")


def test_the_new_struct_matches_the_c_layout():
    fields = [f[0] for f in _lib.BtsLossRegArgs._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bts_render.h"\nint main(void) {\n  printf("%zu", sizeof(BtsLossRegArgs));\n' + \
        "".join(f'  printf(" %zu", offsetof(BtsLossRegArgs, {f}));\n' for f in fields) + '  printf(" %d", BTS_ABI_VERSION);\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.BtsLossRegArgs) == 152
    assert out[1:-1] == [getattr(_lib.BtsLossRegArgs, f).offset for f in fields]
    assert out[-1] == _lib.ABI_VERSION == 9


def test_symbols_export_and_the_abi_version_stays(lib):
    for name in ("bts_loss_regularisers", "bts_loss_regularisers_workspace"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.bts_abi_version() == _lib.ABI_VERSION == 9
    assert native.loss_regularisers and native.loss_regularisers_packed


def test_workspace_size_is_positive_and_monotone(lib):
    ws = lib.bts_loss_regularisers_workspace
    assert ws(64, 1, 8, 8, 8) > 0 and ws(192 * 640, 1, 192, 640, 64) > 0 and ws(35, 1, 5, 7, 130) > 0
    for bad in ((0, 1, 8, 8, 8), (64, 0, 8, 8, 8), (64, 1, 0, 8, 8), (64, 1, 8, 0, 8), (64, 1, 8, 8, 1), (64, 1, 8, 8, 257), (65, 1, 8, 8, 8)):
        assert ws(*bad) == 0, bad
    for a, b in (((64, 1, 8, 8, 8), (128, 2, 8, 8, 8)), ((2880, 1, 40, 72, 64), (5760, 2, 40, 72, 64)),
                 ((16 * 4096, 1024, 8, 8, 64), (32 * 4096, 2048, 8, 8, 64)), ((4, 1, 2, 2, 64), (8, 2, 2, 2, 64))):
        assert 0 < ws(*a) <= ws(*b), (a, b)


def _args(B=384, n_patches=6, ph=8, pw=8, nv=3, K=8, Ki=5, policy=1, coef=(0.1, 0.1, 0.1, 0.1), **ptrs):
    """A BtsLossRegArgs whose pointers are non-NULL dummies: the calls below must fail before anything is read or launched."""
    d = dict(alphas=16, depth=16, weights=16, invalid=16, invalid_wsum=None, invalid_any=None, rgb_samps=16, terms=16, reg=16, g_alphas=None,
             g_depth=None)
    d.update(ptrs)
    return _lib.BtsLossRegArgs(B=B, n_patches=n_patches, patch_h=ph, patch_w=pw, nv=nv, K=K, K_invalid=Ki, invalid_policy=policy,
                               alpha_reg_slice=0, alpha_reg_fraction=0.125, coef_alpha_reg=coef[0], coef_surfaceness=coef[1],
                               coef_entropy=coef[2], coef_depth=coef[3], **d)


def test_argument_errors_are_codes_with_messages(lib):
    need = lib.bts_loss_regularisers_workspace(384, 6, 8, 8, 8)
    call = lambda a, ws=16, nbytes=need: lib.bts_loss_regularisers(C.byref(a) if a is not None else None, ws, nbytes, None)
    err = lambda: lib.bts_last_error()
    assert call(None) == E_INVALID and b"bts_loss_regularisers" in err() and b"NULL required pointer" in err()
    for k in ("alphas", "terms", "reg", "depth"):
        assert call(_args(**{k: None})) == E_INVALID and b"NULL required pointer" in err(), k
    # without the depth term depth may be NULL, without an alpha term alphas: the next check (here the workspace's) answers
    assert call(_args(depth=None, coef=(0.1, 0, 0, 0)), nbytes=0) == E_INVALID and b"workspace too small" in err()
    assert call(_args(alphas=None, coef=(0, 0, 0, 0.1)), nbytes=0) == E_INVALID and b"workspace too small" in err()
    for k in ("B", "n_patches", "ph", "pw", "K"):
        assert call(_args(**{k: 0})) == E_INVALID and b"non-positive size" in err(), k
        assert call(_args(**{k: -3})) == E_INVALID and b"non-positive size" in err(), k
    assert call(_args(nv=0)) == E_INVALID and b"non-positive size" in err()
    assert call(_args(K=1)) == E_UNSUPPORTED and b"K = 1 samples per ray are outside [2, 256]" in err()
    assert call(_args(K=257)) == E_UNSUPPORTED and b"K = 257 samples per ray are outside [2, 256]" in err()
    assert call(_args(B=48, ph=1, pw=8)) == E_UNSUPPORTED and b"the depth term needs patch_h >= 2 and patch_w >= 2, got 1 x 8" in err()
    assert call(_args(B=48, ph=8, pw=1)) == E_UNSUPPORTED and b"got 8 x 1" in err() and b"NaN" in err()
    assert call(_args(B=48, ph=1, pw=8, coef=(0.1, 0.1, 0.1, 0)), nbytes=0) == E_INVALID and b"workspace" in err()      # no depth term: fine so far
    assert call(_args(B=385)) == E_INVALID and b"B = 385 rays are not n_patches * patch_h * patch_w = 384" in err()
    assert call(_args(B=(1 << 29) + 64, n_patches=(1 << 23) + 1)) == E_INVALID and b"2^29" in err()
    for p in (-1, 4):
        assert call(_args(policy=p)) == E_INVALID and b"unknown invalid_policy" in err(), p
    for k in ("rgb_samps", "weights", "invalid"):
        assert call(_args(policy=3, **{k: None})) == E_INVALID and b"weight_guided_diverse needs rgb_samps, weights and invalid" in err(), k
    assert call(_args(policy=1, invalid=None)) == E_INVALID and b"invalid_policy 1 needs" in err()
    assert call(_args(policy=2, weights=None)) == E_INVALID and b"invalid_policy 2 needs" in err()
    assert call(_args(policy=2, Ki=0)) == E_INVALID and b"invalid_policy 2 needs" in err()
    assert call(_args(g_alphas=16, coef=(0, 0, 0, 0.1))) == E_INVALID and b"g_alphas needs an alpha term" in err()
    assert call(_args(g_depth=16, coef=(0.1, 0, 0, 0))) == E_INVALID and b"g_depth the depth term" in err()
    assert call(_args(), nbytes=need - 1) == E_INVALID and b"workspace too small" in err()
    assert call(_args(), ws=None) == E_INVALID and b"workspace too small" in err()


@pytest.mark.parametrize("cname", list(RO.CONFIGS))
@pytest.mark.parametrize("layout", list(RO.LAYOUTS))
def test_the_restatement_reproduces_the_reference(golden, layout, cname):
    z = golden
    levels, gt = RO.load_inputs(z, layout)
    L = RO.LAYOUTS[layout]
    assert len(levels) == L["S"] and levels[0]["alphas"].shape == (L["n"], L["pc"], L["h"], L["w"], L["K"])
    lv, leaves = RO.leaves(levels)
    loss, d, _ = RO.reconstruction_loss(lv, gt, RO.config_of(cname))
    g = RO.grads(loss, leaves)
    key = f"{layout}_{cname}"
    want = dict(zip(RO.DICT_KEYS, z[f"{key}_loss_dict"].tolist()))
    assert abs(loss.item() - z[f"{key}_loss"].item()) <= 1e-6
    for k in RO.DICT_KEYS:
        assert abs(d[k] - want[k]) <= 1e-6 * max(1.0, abs(want[k])), k
    for s in range(L["S"]):
        for got, ref in ((g[2 * s], z[f"{key}_g_alphas_{s}"]), (g[2 * s + 1], z[f"{key}_g_depth_{s}"])):
            ref = torch.from_numpy(ref)
            assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_the_golden_is_small_and_carries_its_constructed_blocks(golden):
    assert os.path.getsize(RO.GOLDEN) < 400_000
    levels, gt = RO.load_inputs(golden, "p8")
    a = levels[0]["alphas"]
    s, p, rows = RO.TIE_BLOCK
    assert (a[s, p, rows][..., :-1].sum(-1) == 1.0).all() and (a[s, p, rows][..., -1] == 1.0).all()
    s, p, y = RO.CARRIED_ROW
    A = a[s, p, y][..., :-1].sum(-1)
    assert (A > 1).sum() == 1 and (A - 1).sum() > 0.5
    assert all((lv[0]["alphas"] == 0).any() and (lv[0]["alphas"] == 1).any() for lv in (RO.load_inputs(golden, k)[0] for k in RO.LAYOUTS))
    # the tie takes the full gradient: keep * lambda / n_scales / B, in the reference's own numbers
    g = torch.from_numpy(golden["p8_alpha_ray_g_alphas_0"])
    B = a[..., 0].numel()
    tie = g[RO.TIE_BLOCK[0], RO.TIE_BLOCK[1], RO.TIE_BLOCK[2]]
    assert (tie[..., :-1] / (0.05 / 3 / B) - 1).abs().max() <= 3e-7 and (tie[..., -1] == 0).all()


def test_the_mutants_differ_from_the_restatement(golden):
    levels, gt = RO.load_inputs(golden, "p8")
    base, d0, _ = RO.reconstruction_loss(levels, gt, RO.config_of("all_strict_lean"))
    for m in ("last_in_sum", "cap_k_minus_1", "cap_unmasked", "entropy_log2", "entropy_unmasked", "entropy_scaled", "surf_mask_never",
              "depth_masked", "depth_borders"):
        other, _, _ = RO.reconstruction_loss(levels, gt, RO.config_of("all_strict_lean"), mutant=m)
        assert abs(other.item() - base.item()) > 1e-5, m
