"""CPU (no GPU, no kernel launches): which invalid-ray inputs reach the library.  Part one: the four loss entry points of
``behindthescenes_amd.native`` against a recording stand-in for the library -- per policy and per form of the inputs (per-sample
tensors, the renderer's per-ray sums, both) which pointer fields of the argument struct are NULL and what K / K_invalid / nv /
invalid_policy say.  Part two: ``ReconstructionLoss`` against recording stand-ins for those entry points -- what scale 0's render dict
(full, lean, diverse) becomes on its way down, and that the diverse flags are launched once per call.  Every expectation is a literal."""
import ctypes as C
import inspect

import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import native

MASKS = ("weights", "invalid", "invalid_wsum", "invalid_any", "rgb_samps")
B, K, NV = 32, 3, 2      # two 4 x 4 patches


class _OnGpu(torch.Tensor):
    """a CPU tensor that passes the entry points' GPU check (its data_ptr is real, nothing reads it)"""
    is_cuda = property(lambda self: True)


class _Lib:
    """records (symbol, arguments); every call succeeds, every workspace is 64 bytes"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 64 if name.endswith("_workspace") else 0
        return fn

    def struct(self, symbol):
        (args,) = [a for n, a in self.calls if n == symbol]
        return args[0]._obj


@pytest.fixture
def lib(monkeypatch):
    rec = _Lib()
    monkeypatch.setattr(native._lib, "load", lambda: rec)
    monkeypatch.setattr(native, "_stream", lambda t: None)
    return rec


def _t(*shape):
    return torch.rand(*shape).as_subclass(_OnGpu)


def _given(form, diverse=False):
    kw = {}
    if form in ("samples", "both"):
        kw.update(weights=_t(B, K), invalid=_t(B, K, NV))
        if diverse:
            kw.update(rgb_samps=_t(B, K, NV, 3))
    if form in ("sums", "both"):
        kw.update(invalid_wsum=_t(B, NV), invalid_any=_t(B, NV))
    return kw


# (policy, form) -> the pointer fields that are not NULL, the struct's policy, the sample count the struct carries for the masks
EXPECT = {
    ("none", "samples"): (set(), 0, 0), ("none", "sums"): (set(), 0, 0), ("none", "both"): (set(), 0, 0),
    (None, "samples"): (set(), 0, 0), (None, "sums"): (set(), 0, 0),
    ("strict", "samples"): ({"invalid"}, 1, K), ("strict", "sums"): ({"invalid_any"}, 1, 0), ("strict", "both"): ({"invalid_any"}, 1, 0),
    ("weight_guided", "samples"): ({"weights", "invalid"}, 2, K), ("weight_guided", "sums"): ({"invalid_wsum"}, 2, 0),
    ("weight_guided", "both"): ({"invalid_wsum"}, 2, 0),
    ("weight_guided_diverse", "samples"): ({"weights", "invalid", "rgb_samps"}, 3, K),
    ("weight_guided_diverse", "both"): ({"weights", "invalid", "rgb_samps"}, 3, K),
}
L1SSIM = [k for k in EXPECT if k[0] != "weight_guided_diverse"]


def _check(a, given, policy, form, k_field="K", nv=NV):
    live, pol, k = EXPECT[(policy, form)]
    for f in MASKS:
        if not hasattr(a, f):
            assert f == "rgb_samps"      # (BtsLossArgs: the l1+ssim entries know no diverse policy)
            continue
        assert getattr(a, f) == (given[f].data_ptr() if f in live else None), (f, policy, form)
    assert (a.invalid_policy, getattr(a, k_field), a.nv) == (pol, k, nv)


@pytest.mark.parametrize("policy,form", L1SSIM)
def test_photometric_loss_hands_down_what_the_policy_reads(lib, policy, form):
    given = _given(form)
    rgb, depth, gt = _t(B, NV * 3), _t(B), _t(B, 3)
    parts, g_rgb, g_depth = native.photometric_loss(rgb, depth, given.get("weights"), given.get("invalid"), gt, 4, 4, policy, False, 1.0, 1.0,
                                                    invalid_wsum=given.get("invalid_wsum"), invalid_any=given.get("invalid_any"))
    a = lib.struct("bts_photometric_loss")
    _check(a, given, policy, form)
    assert (a.n_patches, a.patch_h, a.patch_w, a.edge_aware_smoothness) == (2, 4, 4, 0) and parts.shape == (2, 4)
    # depth is handed over, and gets its gradient, whenever it is given -- with or without the smoothness term
    assert a.depth == depth.data_ptr() and a.g_depth == g_depth.data_ptr() and a.g_rgb == g_rgb.data_ptr() and a.rgb == rgb.data_ptr()
    assert (a.rgb_gt, a.parts) == (gt.data_ptr(), parts.data_ptr())


def test_photometric_loss_routes_large_patches_and_the_bound(lib):
    rgb, gt, thr = _t(256, 3), _t(256, 3), _t(256)
    native.photometric_loss(rgb, None, None, None, gt, 16, 16, "none", False, 1.0, 1.0, need_grad=False, thresh=thr)
    assert [n for n, _ in lib.calls] == ["bts_photometric_loss_tiled_automask_workspace", "bts_photometric_loss_tiled_automask"]
    a = lib.struct("bts_photometric_loss_tiled_automask")
    assert (a.depth, a.g_rgb, a.g_depth, a.nv, a.K, a.n_patches) == (None, None, None, 1, 0, 1)
    with pytest.raises(KeyError):
        native.photometric_loss(rgb, None, None, None, gt, 16, 16, "weight_guided_diverse", False, 1.0, 1.0)


@pytest.mark.parametrize("policy,form", L1SSIM)
def test_photometric_loss_median_hands_down_what_the_policy_reads(lib, policy, form):
    given = _given(form)
    rgb, depth, gt, parts = _t(B, NV * 3), _t(B), _t(B, 3), _t(2, 4)      # (parts: the entry checks the one it allocates like a given one)
    for eas in (False, True):
        lib.calls.clear()
        out, thresholds, kept, g_rgb, g_depth = native.photometric_loss_median(
            rgb, depth, given.get("weights"), given.get("invalid"), gt, 2, 4, 4, policy, eas, invalid_wsum=given.get("invalid_wsum"),
            invalid_any=given.get("invalid_any"), parts=parts)
        a = lib.struct("bts_photometric_loss_median")
        _check(a, given, policy, form)
        assert a.parts == parts.data_ptr() and a.n_patches == 2
        # ... while the median form hands depth over only with the smoothness term
        assert a.depth == (depth.data_ptr() if eas else None) and (g_depth is not None) == eas and a.g_depth == (g_depth.data_ptr() if eas else None)
        assert a.edge_aware_smoothness == int(eas) and a.g_rgb == g_rgb.data_ptr() and (out.shape, thresholds.shape, kept.dtype) == ((4,), (2,), torch.int64)
    with pytest.raises(bts.BtsNativeError, match="is not one of none / strict / weight_guided"):
        native.photometric_loss_median(rgb, depth, None, None, gt, 2, 4, 4, "weight_guided_diverse", False)


@pytest.mark.parametrize("policy,form", list(EXPECT))
def test_pixel_loss_hands_down_what_the_policy_reads(lib, policy, form):
    given = _given(form, diverse=True)
    rgb, depth, gt = _t(B, NV * 3), _t(B), _t(B, 3)
    out, thresholds, kept, g_rgb, g_depth = native.pixel_loss(rgb, depth, given.get("weights"), given.get("invalid"), gt, 2, 4, 4, "l1", policy, True,
                                                              False, invalid_wsum=given.get("invalid_wsum"),
                                                              invalid_any=given.get("invalid_any"), rgb_samps=given.get("rgb_samps"))
    a = lib.struct("bts_pixel_loss")
    _check(a, given, policy, form)
    assert (a.B, a.n, a.criterion, a.median_thresholding, a.depth, a.g_depth, g_depth) == (B, 2, 1, 1, None, None, None)
    assert a.thresholds == thresholds.data_ptr() and a.kept == kept.data_ptr() and a.g_rgb == g_rgb.data_ptr()


@pytest.mark.parametrize("policy,form", list(EXPECT))
def test_loss_regularisers_hand_down_what_the_policy_reads(lib, policy, form):
    given = _given(form, diverse=True)
    alphas, depth = _t(B, 6), _t(B)
    terms, reg, g_alphas, g_depth, out = native.loss_regularisers_packed(alphas, depth, n=1, pc=2, ph=4, pw=4, policy=policy, coef=(0.1, 0, 0, 0),
                                                                         **given)
    a = lib.struct("bts_loss_regularisers")
    _check(a, given, policy, form, k_field="K_invalid", nv=NV if EXPECT[(policy, form)][1] else 0)
    assert (a.B, a.n_patches, a.K, a.depth, a.g_depth, g_depth) == (B, 2, 6, None, None, None)
    assert a.alphas == alphas.data_ptr() and a.g_alphas == g_alphas.data_ptr() and a.terms == out.data_ptr() and a.reg == out.data_ptr() + 20


def test_the_two_policy_tables_are_one():
    assert native.PIXEL_POLICIES == {None: 0, "none": 0, "strict": 1, "weight_guided": 2, "weight_guided_diverse": 3}
    assert native.INVALID_POLICIES == {None: 0, "none": 0, "strict": 1, "weight_guided": 2}
    assert list(native.INVALID_POLICIES.items()) == list(native.PIXEL_POLICIES.items())[:4]


def test_a_wrong_shape_is_still_named(lib):
    rgb, gt = _t(B, NV * 3), _t(B, 3)
    with pytest.raises(bts.BtsNativeError, match=r"invalid_wsum / invalid_any: expected shape \(32, 2\)"):
        native.photometric_loss(rgb, None, None, None, gt, 4, 4, "strict", False, 1.0, 1.0, invalid_any=_t(B, 3))
    with pytest.raises(bts.BtsNativeError, match=r"weights: expected shape \(32, 3\)"):
        native.pixel_loss(rgb, None, _t(B, 4), _t(B, K, NV), gt, 2, 4, 4, "l2", "weight_guided", False, False)
    with pytest.raises(bts.BtsNativeError, match=r"rgb_samps: expected shape \(32, 3, 2, 3\)"):
        native.loss_regularisers(_t(B, 6), None, n=1, pc=2, ph=4, pw=4, policy="weight_guided_diverse", coef=(0.1, 0, 0, 0), weights=_t(B, K),
                                 invalid=_t(B, K, NV), rgb_samps=_t(B, K, NV * 3))
    assert lib.calls == []


# --------------------------------------------------------------------------------------------------------------
# ReconstructionLoss: scale 0's render dict on its way to the entry points
# --------------------------------------------------------------------------------------------------------------
N, PC, H, W = 1, 2, 4, 4


class _Native:
    """records the entry points' arguments by parameter name (however they were passed) and answers with tensors of the right shapes"""

    def __init__(self, monkeypatch):
        self.calls = {}
        self.flags = []
        for name in ("photometric_loss", "photometric_loss_median", "pixel_loss", "loss_regularisers_packed", "loss_diverse_flags"):
            monkeypatch.setattr(native, name, self._fake(name, inspect.signature(getattr(native, name))))

    def _fake(self, name, sig):
        def fn(*a, **k):
            args = sig.bind(*a, **k)
            args.apply_defaults()
            self.calls.setdefault(name, []).append(args.arguments)
            if name == "loss_diverse_flags":
                self.flags.append(torch.zeros(B, NV))
                return self.flags[-1]
            if name == "loss_regularisers_packed":
                out = torch.zeros(6)
                return out[:5], out[5:], None, None, out
            if name == "photometric_loss":
                return torch.zeros(PC, 4), None, None
            return torch.zeros(4), None, None, None, None
        return fn


def _dicts(form, S=2, alphas=False):
    g = torch.Generator().manual_seed(0)
    if form == "lean":
        masks = dict(invalid_wsum=torch.rand(N, PC, H, W, NV, generator=g), invalid_any=torch.rand(N, PC, H, W, NV, generator=g))
    else:
        masks = dict(weights=torch.rand(N, PC, H, W, K, generator=g), invalid=torch.rand(N, PC, H, W, K, NV, generator=g))
        if form == "diverse":
            masks["rgb_samps"] = torch.rand(N, PC, H, W, K, NV, 3, generator=g)
    levels = []
    for _ in range(S):
        lv = dict(masks, rgb=torch.rand(N, PC, H, W, NV, 3, generator=g), depth=torch.rand(N, PC, H, W, generator=g) + 1)
        if alphas:
            lv["alphas"] = torch.rand(N, PC, H, W, K, generator=g)
        levels.append(lv)
    return levels, dict(coarse=levels, fine=[dict(lv) for lv in levels], rgb_gt=torch.rand(N, PC, H, W, 3, generator=g))


# (policy, form of the dict) -> the masks that arrive (the dict's own memory, flat), every other one None
ARRIVE = {
    ("none", "full"): (), (None, "lean"): (), ("none", "lean"): (),
    ("strict", "full"): ("invalid",), ("strict", "lean"): ("invalid_any",),
    ("weight_guided", "full"): ("weights", "invalid"), ("weight_guided", "lean"): ("invalid_wsum",),
}
FLAT = dict(weights=(B, K), invalid=(B, K, NV), invalid_wsum=(B, NV), invalid_any=(B, NV), rgb_samps=(B, K, NV, 3))


def _check_masks(got, level0, live, names=MASKS):
    for f in names:
        if f in live:
            assert got[f].data_ptr() == level0[f].data_ptr() and got[f].shape == FLAT[f] and not got[f].requires_grad, f
        else:
            assert got[f] is None, f


@pytest.mark.parametrize("policy,form", list(ARRIVE))
@pytest.mark.parametrize("median", [False, True])
def test_sums_hand_scale_0s_masks_to_every_scale(monkeypatch, policy, form, median):
    rec = _Native(monkeypatch)
    levels, data = _dicts(form)
    crit = bts.ReconstructionLoss(dict(criterion="l1+ssim", invalid_policy=policy, lambda_edge_aware_smoothness=0.001,
                                       median_thresholding=median, native_ssim_median=True))
    crit(data)
    calls = rec.calls.pop("photometric_loss_median" if median else "photometric_loss")
    assert len(calls) == 2 and rec.calls == {}      # (the fine dicts alias the coarse ones: one launch per scale)
    for s, a in enumerate(calls):
        _check_masks(a, levels[0], ARRIVE[(policy, form)], MASKS[:4])
        assert a["invalid_policy"] == policy and a["eas"] is True and (a["patch_h"], a["patch_w"], a["thresh"]) == (H, W, None)
        assert a["rgb"].data_ptr() == levels[s]["rgb"].data_ptr() and a["rgb"].shape == (B, NV * 3)
        assert a["depth"].data_ptr() == levels[s]["depth"].data_ptr() and a["rgb_gt"].data_ptr() == data["rgb_gt"].data_ptr()
        assert (a["scale_rgb"], a["scale_eas"]) == (1.0, 1.0) and a["need_grad"] is False
        if median:
            assert a["n"] == N


@pytest.mark.parametrize("policy,form", list(ARRIVE) + [("weight_guided_diverse", "diverse")])
@pytest.mark.parametrize("median", [False, True])
def test_pixel_hands_scale_0s_masks_to_every_scale(monkeypatch, policy, form, median):
    rec = _Native(monkeypatch)
    levels, data = _dicts(form)
    crit = bts.ReconstructionLoss(dict(criterion="l1", invalid_policy=policy, median_thresholding=median, native_pixel_loss=True))
    crit(data)
    calls = rec.calls.pop("pixel_loss")
    assert len(calls) == 2 and rec.calls == {}      # (the diverse policy reads the per-sample tensors itself: no flags launch)
    live = ("rgb_samps", "weights", "invalid") if form == "diverse" else ARRIVE[(policy, form)]
    for s, a in enumerate(calls):
        _check_masks(a, levels[0], live)
        assert (a["invalid_policy"], a["criterion"], a["median"], a["eas"], a["depth"], a["n"]) == (policy, "l1", median, False, None, N)
        assert a["rgb"].data_ptr() == levels[s]["rgb"].data_ptr() and (a["patch_h"], a["patch_w"]) == (H, W)


@pytest.mark.parametrize("policy,form", list(ARRIVE))
def test_regularisers_hand_scale_0s_masks_to_every_scale(monkeypatch, policy, form):
    rec = _Native(monkeypatch)
    levels, data = _dicts(form, alphas=True)
    crit = bts.ReconstructionLoss(dict(criterion="l1+ssim", invalid_policy=policy, lambda_alpha_reg=0.1, native_regularisers=True))
    crit(data)
    assert len(rec.calls["photometric_loss"]) == 2
    for s, a in enumerate(rec.calls["loss_regularisers_packed"]):
        _check_masks(a, levels[0], ARRIVE[(policy, form)])
        assert a["policy"] == (policy or "none") and (a["n"], a["pc"], a["ph"], a["pw"]) == (N, PC, H, W) and a["coef"] == (0.05, 0.0, 0.0, 0.0)
        assert a["alphas"].data_ptr() == levels[s]["alphas"].data_ptr() and a["depth"] is None
    assert len(rec.calls["loss_regularisers_packed"]) == 2 and "loss_diverse_flags" not in rec.calls


def test_the_diverse_flags_are_launched_once_per_call_and_go_in_under_strict(monkeypatch):
    rec = _Native(monkeypatch)
    levels, data = _dicts("diverse", alphas=True)
    crit = bts.ReconstructionLoss(dict(criterion="l1+ssim", invalid_policy="weight_guided_diverse", native_pixel_loss=True,
                                       lambda_alpha_reg=0.1, native_regularisers=True))
    for call in (1, 2):
        crit(data)
        assert len(rec.calls["loss_diverse_flags"]) == call == len(rec.flags)      # two scales, photometric term and regularisers: one launch
        _check_masks(rec.calls["loss_diverse_flags"][-1], levels[0], ("rgb_samps", "weights", "invalid"), ("rgb_samps", "weights", "invalid"))
        sums, regs = rec.calls["photometric_loss"][-2:], rec.calls["loss_regularisers_packed"][-2:]
        for a in sums + regs:
            assert a["invalid_any"] is rec.flags[-1] and a["weights"] is None and a["invalid"] is None and a["invalid_wsum"] is None
        assert [a["invalid_policy"] for a in sums] == ["strict"] * 2 and [a["policy"] for a in regs] == ["strict"] * 2
        assert all(a["rgb_samps"] is None for a in regs)
    # without the regularisers too, through the one-matrix path
    rec.calls.clear()
    bts.ReconstructionLoss(dict(criterion="l1+ssim", invalid_policy="weight_guided_diverse", native_pixel_loss=True))(data)
    assert len(rec.calls["loss_diverse_flags"]) == 1 and [a["invalid_any"] is rec.flags[-1] for a in rec.calls["photometric_loss"]] == [True, True]


def test_a_lean_dict_under_the_diverse_policy_says_what_to_ask_the_renderer_for(monkeypatch):
    rec = _Native(monkeypatch)
    _, data = _dicts("lean")
    for cfg in (dict(criterion="l1+ssim"), dict(criterion="l1")):
        with pytest.raises(KeyError, match="want_rgb_samps=True"):
            bts.ReconstructionLoss(dict(cfg, invalid_policy="weight_guided_diverse", native_pixel_loss=True))(data)
    assert rec.calls == {}


def test_regularisers_on_follows_the_lambdas():
    base = dict(criterion="l1+ssim", invalid_policy="strict")
    assert not bts.ReconstructionLoss(dict(base, lambda_edge_aware_smoothness=0.1)).regularisers_on
    for key in ("lambda_depth_reg", "lambda_alpha_reg", "lambda_surfaceness_reg", "lambda_depth_smoothness", "lambda_entropy"):
        crit = bts.ReconstructionLoss(dict(base, **{key: 0.1}))
        assert crit.regularisers_on
        setattr(crit, key, 0)          # (read per call: a schedule may change a lambda)
        assert not crit.regularisers_on
