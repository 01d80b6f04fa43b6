"""GPU: the opt-in `native_regularisers: true` of ReconstructionLoss -- alpha_reg (ray | slice), surfaceness, ray entropy and the depth
term on bts_loss_regularisers (csrc/bts_loss_reg.hip) -- against tests/golden/loss_reg.npz (the REAL reference's ReconstructionLoss on
four layouts and nine configurations, tests/golden/gen_golden_loss_reg.py) and the CPU restatement tests/_loss_reg_oracle.py (pinned
to that golden in tests/test_loss_reg_cpu.py).  The project's bars: loss within 1e-5, each logged term 1e-5 relative, invalid ratio
1e-6, d loss / d alphas and d loss / d depth within 1e-4 of the largest entry; the tie block's gradients are exactly keep * c / B.  The
golden's generator asserts that the fp32 reference is within a tenth of these bars of its fp64 evaluation, that no gate outside the tie
block is closer than 1e-3 to 0, and that each mutant of the restatement leaves the bars.  Measured on MI355X over the 36 cases: the
new path's gradients are at most 3.0e-7 of the largest entry from the reference's, the torch composition's (no key) 4.2e-7; end to end
the parameter gradients with and without the key differ by at most 3.7e-7."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _loss_reg_oracle as RO

pytestmark = pytest.mark.gpu
KEY = {"native_regularisers": True}
_CACHE = {}


def _golden(layout):
    """the layout's inputs (CPU tensors), loaded once and left unchanged"""
    if "z" not in _CACHE:
        _CACHE["z"] = np.load(RO.GOLDEN)
    if layout not in _CACHE:
        _CACHE[layout] = RO.load_inputs(_CACHE["z"], layout)
    return _CACHE["z"], _CACHE[layout][0], _CACHE[layout][1]


def _hip(levels_cpu, gt, config, lean=False, grad=True):
    """ReconstructionLoss on the GPU -> loss, dict, [d alphas_0, d depth_0, d alphas_1, ...] (None where nothing flowed)"""
    import behindthescenes_amd as bts
    dev, leaves = [], []
    for s, lv in enumerate(levels_cpu):
        src = RO.lean_of(lv) if lean else lv
        d = {k: v.cuda() for k, v in src.items()}
        d["alphas"], d["depth"] = d["alphas"].requires_grad_(grad), d["depth"].requires_grad_(grad)
        dev.append(d)
        leaves += [d["alphas"], d["depth"]]
    crit = bts.ReconstructionLoss(dict(config))
    loss, parts = crit(dict(coarse=dev, fine=[dict(d) for d in dev], rgb_gt=gt.cuda()))
    if grad:
        loss.backward()
    return loss, parts, [x.grad for x in leaves]


def _check(got, z, key, S, tag):
    loss, parts, g = got
    want = dict(zip(RO.DICT_KEYS, z[f"{key}_loss_dict"].tolist()))
    assert list(parts) == RO.DICT_KEYS
    print(tag, "loss", loss.item(), z[f"{key}_loss"].item(), {k: (parts[k], want[k]) for k in RO.TERM_KEYS}, "invalid",
          parts["loss_invalid_ratio"], want["loss_invalid_ratio"])
    errs = {}
    for s in range(S):
        for name, got_g in ((f"alphas_{s}", g[2 * s]), (f"depth_{s}", g[2 * s + 1])):
            ref = torch.from_numpy(z[f"{key}_g_{name}"])
            if ref.abs().max() == 0:
                assert got_g is None or not got_g.any(), name           # a term that is off hands on nothing
                continue
            errs[name] = (got_g.cpu() - ref).abs().max().item() / ref.abs().max().item()
    print(tag, "gradient errors", errs)
    assert abs(loss.item() - z[f"{key}_loss"].item()) <= 1e-5, (loss.item(), z[f"{key}_loss"].item())
    assert abs(parts["loss"] - want["loss"]) <= 1e-5
    for k in RO.TERM_KEYS:
        assert abs(parts[k] - want[k]) <= 1e-5 * abs(want[k]), (k, parts[k], want[k])
    for k in ("loss_rgb_coarse", "loss_rgb_fine"):
        assert abs(parts[k] - want[k]) <= 1e-5, k
    assert abs(parts["loss_invalid_ratio"] - want["loss_invalid_ratio"]) <= 1e-6 and parts["loss_eas"] == 0
    assert errs, "no gradient compared"
    for name, err in errs.items():
        assert err <= 1e-4, (name, err)


@pytest.mark.parametrize("cname", list(RO.CONFIGS))
@pytest.mark.parametrize("layout", list(RO.LAYOUTS))
def test_regularisers_vs_the_real_reference(layout, cname):
    z, levels, gt = _golden(layout)
    got = _hip(levels, gt, dict(RO.config_of(cname), **KEY), lean=cname in RO.LEAN)
    _check(got, z, f"{layout}_{cname}", len(levels), f"{layout} {cname} [native]")


@pytest.mark.parametrize("cname", list(RO.CONFIGS))
@pytest.mark.parametrize("layout", list(RO.LAYOUTS))
def test_the_shipped_torch_composition_meets_the_same_bars(layout, cname):
    z, levels, gt = _golden(layout)
    got = _hip(levels, gt, RO.config_of(cname), lean=cname in RO.LEAN)
    _check(got, z, f"{layout}_{cname}", len(levels), f"{layout} {cname} [torch]")


@pytest.mark.parametrize("cname", ["alpha_ray", "alpha_slice"])
def test_the_tie_block_takes_exactly_the_full_gradient(cname):
    """A == cap on 16 kept rays (two whole rows, which tie as slice rows too): clamp_min passes the gradient, keep * c / B in fp32 with
    c the coefficient the host hands over (lambda / n_scales) -- and 0 for the last sample"""
    _, levels, gt = _golden("p8")
    _, _, g = _hip(levels, gt, dict(RO.config_of(cname), **KEY))
    s, p, rows = RO.TIE_BLOCK
    tie = g[0][s, p, rows].cpu()
    B = levels[0]["depth"].numel()
    want = np.float32(0.05 / len(levels)) / np.float32(B)
    print(cname, "tie block", tie[0, 0].tolist(), "want", want)
    assert torch.equal(tie[..., :-1], torch.full((2, 8, 7), float(want))) and (tie[..., -1] == 0).all()


def _flat(levels, scale, lean=False):
    from behindthescenes_amd import native        # noqa: F401  (the import builds nothing: the library is loaded on first use)
    lv0, lv = levels[0], levels[scale]
    n, pc, h, w, K = lv["alphas"].shape
    nv = lv0["invalid"].shape[-1]
    f = lambda t, *tail: t.reshape((-1,) + tail).float().contiguous().cuda()
    kw = dict(n=n, pc=pc, ph=h, pw=w)
    if lean:
        ln = RO.lean_of(lv0)
        kw.update(invalid_wsum=f(ln["invalid_wsum"], nv), invalid_any=f(ln["invalid_any"], nv))
    else:
        kw.update(weights=f(lv0["weights"], K), invalid=f(lv0["invalid"], K, nv), rgb_samps=f(lv0["rgb_samps"], K, nv, 3))
    return f(lv["alphas"], K), f(lv["depth"]), kw


COEF = (0.05, 0.1, 0.02, 0.05)


@pytest.mark.parametrize("reduction", ["ray", "slice"])
@pytest.mark.parametrize("layout", list(RO.LAYOUTS))
def test_reruns_are_bit_identical_and_lean_inputs_give_identical_results(layout, reduction):
    from behindthescenes_amd import native
    _, levels, _ = _golden(layout)
    a, d, kw = _flat(levels, 0)
    run = lambda **k: native.loss_regularisers(a, d, coef=COEF, alpha_reg_reduction=reduction, **k)
    for policy in ("strict", "weight_guided", "weight_guided_diverse", "none"):
        x, y = run(policy=policy, **kw), run(policy=policy, **kw)
        assert all(torch.equal(p, q) for p, q in zip(x, y)), policy
        assert x[2].abs().max() > 0 and x[3].abs().max() > 0 and torch.isfinite(x[0]).all() and torch.isfinite(x[1]).all()
        assert (x[0][4].item() > 0) == (policy != "none")
        if policy in ("strict", "weight_guided"):
            _, _, lean = _flat(levels, 0, lean=True)
            assert all(torch.equal(p, q) for p, q in zip(x, run(policy=policy, **lean))), policy
    fwd = native.loss_regularisers(a, d, coef=COEF, alpha_reg_reduction=reduction, policy="strict", need_grad=False, **kw)
    ref = run(policy="strict", **kw)
    assert fwd[2] is None and fwd[3] is None and torch.equal(fwd[0], ref[0]) and torch.equal(fwd[1], ref[1])


@pytest.mark.parametrize("reduction", ["ray", "slice"])
@pytest.mark.parametrize("layout", list(RO.LAYOUTS))
def test_every_gradient_element_is_written(layout, reduction):
    """the entry called with buffers pre-filled with NaN: none is left in g_alphas / g_depth / terms / reg"""
    from behindthescenes_amd import _lib, native
    _, levels, _ = _golden(layout)
    a, d, kw = _flat(levels, 0)
    B, K = a.shape
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    g_a, g_d, out = nan(B, K), nan(B), nan(6)
    Ki, nv = kw["invalid"].shape[1:]
    args = _lib.BtsLossRegArgs(alphas=a.data_ptr(), depth=d.data_ptr(), weights=kw["weights"].data_ptr(), invalid=kw["invalid"].data_ptr(),
                               invalid_wsum=None, invalid_any=None, rgb_samps=None, terms=out.data_ptr(), reg=out.data_ptr() + 20,
                               g_alphas=g_a.data_ptr(), g_depth=g_d.data_ptr(), B=B, n_patches=kw["n"] * kw["pc"], patch_h=kw["ph"],
                               patch_w=kw["pw"], nv=nv, K=K, K_invalid=Ki, invalid_policy=2, alpha_reg_slice=int(reduction == "slice"),
                               alpha_reg_fraction=0.125, coef_alpha_reg=COEF[0], coef_surfaceness=COEF[1], coef_entropy=COEF[2],
                               coef_depth=COEF[3])
    lib = _lib.load()
    ws = torch.full((lib.bts_loss_regularisers_workspace(B, kw["n"] * kw["pc"], kw["ph"], kw["pw"], K),), 255, device="cuda", dtype=torch.uint8)
    _lib.check(lib.bts_loss_regularisers(C.byref(args), ws.data_ptr(), ws.numel(), native._stream(a)), "bts_loss_regularisers")
    assert not torch.isnan(g_a).any() and not torch.isnan(g_d).any() and not torch.isnan(out).any()
    ref = native.loss_regularisers(a, d, coef=COEF, alpha_reg_reduction=reduction, policy="weight_guided", weights=kw["weights"],
                                   invalid=kw["invalid"], n=kw["n"], pc=kw["pc"], ph=kw["ph"], pw=kw["pw"])
    assert torch.equal(g_a, ref[2]) and torch.equal(g_d, ref[3]) and torch.equal(out[:5], ref[0])


def test_a_one_pixel_wide_patch_with_the_depth_term_is_unsupported():
    import behindthescenes_amd as bts
    from behindthescenes_amd import native
    a, d = torch.rand(16, 8, device="cuda"), torch.rand(16, device="cuda")
    with pytest.raises(ValueError, match="at least 2 x 2"):
        native.loss_regularisers(a, d, n=1, pc=1, ph=1, pw=16, policy="none", coef=(0, 0, 0, 0.1))
    terms, reg, g_a, g_d = native.loss_regularisers(a, d, n=1, pc=1, ph=1, pw=16, policy="none", coef=(0.1, 0.1, 0.1, 0))    # without it: fine
    assert torch.isfinite(terms).all() and g_d is None and torch.isfinite(g_a).all()
    with pytest.raises(bts.BtsNativeError, match="outside \\[2, 256\\]"):
        native.loss_regularisers(torch.rand(16, 1, device="cuda"), d, n=1, pc=1, ph=4, pw=4, policy="none", coef=(0.1, 0, 0, 0))


def test_end_to_end_render_criterion_backward():
    """one small render with want_alphas (2 x 2 patches of 8 x 8, K = 8), the criterion with the key, backward: the parameter gradients
    against the same step without the key"""
    import behindthescenes_amd as bts
    from behindthescenes_amd import synthetic as S
    n, V, H, W, K = 2, 4, 24, 40, 8
    ids_loss, ids_render = [0, 1], [2, 3]
    scene = S.synthetic_scene(n, V, H, W, 64, seed=5, baseline=0.4, smooth=True)
    torch.manual_seed(4)
    net = bts.BTSNet(S.field_conf(64, 64, 0, H, W))
    net.encoder = bts.FeatureMapEncoder((H, W), 64, num_views=n)
    S.init_mlp_(net.mlp_coarse, seed=7)
    net = net.to("cuda").train()
    renderer = bts.NeRFRenderer.from_conf(dict(n_coarse=K, lindisp=True, hard_alpha_cap=True)).to("cuda").train()
    wrapped = renderer.bind_parallel(net).train()
    sampler = bts.PatchRaySampler(ray_batch_size=128, z_near=3.0, z_far=80.0, patch_size=8)
    images, projs, poses = (scene[k].cuda() for k in ("images", "projs", "poses"))
    images_ip = images * .5 + .5
    patches = (torch.tensor([[0, 1], [1, 0]]), torch.tensor([[3, 16], [0, 9]]), torch.tensor([[5, 32], [17, 0]]))       # view, y0, x0 per sample
    take = lambda t, ids: t[:, ids].contiguous()
    params = [p for p in net.parameters() if p.requires_grad]
    cfg = dict(RO.ALL, criterion="l1+ssim", invalid_policy="weight_guided", alpha_reg_reduction="slice", lambda_edge_aware_smoothness=0.001)

    def step(key):
        for p in params:
            p.grad = None
        net.encode(images, projs, poses, ids_encoder=[0], ids_render=ids_render)
        rays, gt = sampler.sample(take(images_ip, ids_loss), take(poses, ids_loss), take(projs, ids_loss), patches=patches)
        torch.manual_seed(11)                                      # the jitter of sample_coarse
        rd = wrapped(rays, want_weights=True, want_alphas=True)
        rd["fine"] = dict(rd["coarse"])
        rd["rgb_gt"] = gt
        rd = sampler.reconstruct(rd)
        assert rd["coarse"]["alphas"].shape == (2, 2, 8, 8, K)
        loss, parts = bts.ReconstructionLoss(dict(cfg, **key))(dict(coarse=[rd["coarse"]], fine=[rd["fine"]], rgb_gt=rd["rgb_gt"]))
        loss.backward()
        return loss.item(), dict(parts), [None if p.grad is None else p.grad.clone() for p in params]

    l0, p0, g0 = step({})
    l1, p1, g1 = step(KEY)
    print("end to end: loss", l1, l0, {k: (p1[k], p0[k]) for k in RO.TERM_KEYS})
    assert abs(l1 - l0) <= 1e-5 and all(abs(p1[k] - p0[k]) <= 1e-5 * abs(p0[k]) for k in RO.TERM_KEYS)
    assert p1["loss_alpha_reg"] > 0 and p1["loss_ray_entropy"] > 0 and p1["loss_depth_reg"] > 0
    compared = 0
    for a, b in zip(g1, g0):
        assert (a is None) == (b is None)
        if b is not None and b.abs().max() > 0:
            err = (a - b).abs().max().item() / b.abs().max().item()
            print("parameter gradient", tuple(b.shape), "error", err)
            assert err <= 1e-4
            compared += 1
    assert compared >= 2
