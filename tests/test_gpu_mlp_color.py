"""MLP-predicted colour (``sample_color: false``) on the HIP kernels (``native_mlp_color: true``): bts_field_query_mlp_color,
bts_render_fwd_mlp_color and bts_render_bwd_mlp_color against the PyTorch composition of torch_modes.py evaluated in fp32 on the CPU, as the reference computes
(itself pinned to the reference's outputs by tests/test_torch_modes.py), at the envelope's shapes."""
import copy

import pytest
import torch

import behindthescenes_amd as bts
from oracle import bts_oracle as O
from tests._hip_helpers import make_conf

pytestmark = pytest.mark.gpu

SHAPES = [  # (C, Hd, n_blocks, code_mode, learn_empty, empty_empty)
    (64, 64, 0, "z", True, False),
    (32, 32, 1, "distance", False, True),
]


def _close(got, f32, f64, mask=None, name="", slack=2e-6):
    """The rule of tests/test_gpu_fused_anchor.py::_check_grads: no further from fp64 than the fp32 composition is (x 1.5 + slack), in
    max-norm and L2, over the entries of ``mask``."""
    got, f32, f64 = got.detach().cpu().double(), f32.detach().cpu().double(), f64.detach().cpu().double()
    if mask is not None:
        got, f32, f64 = got[mask], f32[mask], f64[mask]
    e_n, e_t = (got - f64).abs().max().item(), (f32 - f64).abs().max().item()
    l_n, l_t = (got - f64).norm().item(), (f32 - f64).norm().item()
    print(f"  {name}: max err {e_n:.2e} (fp32 composition {e_t:.2e}), L2 {l_n:.2e} ({l_t:.2e}), max |x| {f64.abs().max().item():.2e}")
    assert e_n <= 1.5 * e_t + slack and l_n <= 1.5 * l_t + slack * max(1.0, got.numel() ** 0.5), name


def _nets(C, Hd, nb, code_mode, learn_empty, empty_empty, n=2, H=24, W=40, seed=0, fs=0):
    cfg = O.FieldConfig()
    cfg.code_mode, cfg.learn_empty, cfg.empty_empty = code_mode, learn_empty, empty_empty
    scene = O.synthetic_scene(n, 3, H, W, C, seed=seed, smooth=True)
    conf = make_conf(cfg, C, Hd, nb, H, W)
    conf["sample_color"] = False
    if fs:   # a second decoder scale at half size: rendered through feat_shift 1 (the composition resizes it, models_bts.py:115-117)
        conf["encoder"] = dict(conf["encoder"], n_scales=2, pyramid=True)
    g = torch.Generator().manual_seed(seed + 1)
    torch.manual_seed(seed)   # (the modules' own initialisation -- the second scale's map, the empty feature -- draws from the global generator)
    ref = bts.BTSNet(dict(conf))
    with torch.no_grad():
        for p in ref.mlp_coarse.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.1))
        # a visible share of samples with a dead density (o0 < 0) and a live colour gradient
        ref.mlp_coarse.lin_out.bias[0] = -0.4
        ref.encoder.feats[0].data = scene["feat"].clone()
        if learn_empty:
            ref.empty_feature.copy_(torch.randn(C, generator=g))
    nat = bts.BTSNet(dict(conf, native_mlp_color=True))
    nat.encoder.feats[0].data = scene["feat"].clone()
    nat.load_state_dict(ref.state_dict())
    ref = ref.float()   # the reference computes in fp32: its frustum flags are the contract
    nat = nat.cuda()
    r64 = copy.deepcopy(ref).double()     # fp64 truth: the yardstick of the fp32 errors
    ref.encode(scene["images"], scene["projs"], scene["poses"], ids_encoder=[0], ids_render=[1, 2])
    ref.__dict__["r64"] = r64   # (not a child module: the two nets keep their own dtypes)
    ref.r64.encode(scene["images"].double(), scene["projs"].double(), scene["poses"].double(), ids_encoder=[0], ids_render=[1, 2])
    nat.encode(scene["images"].cuda(), scene["projs"].cuda(), scene["poses"].cuda(), ids_encoder=[0], ids_render=[1, 2])
    rays = O.image_rays(scene["poses"], scene["projs"], H, W, cfg.d_min, cfg.d_max)[:, ::7].contiguous()
    for m in (ref, ref.r64, nat):
        m.set_scale(fs)
    return ref, nat, rays, cfg, g


@pytest.mark.parametrize("shape", SHAPES)
def test_field_query_vs_torch_composition(shape):
    ref, nat, rays, cfg, g = _nets(*shape)
    assert not nat.torch_mode and ref.torch_mode
    n = rays.shape[0]
    K = 16
    z = O.sample_coarse(rays.reshape(-1, 8), K, True, torch.rand(rays.shape[0] * rays.shape[1], K, generator=g))
    pts = (rays.reshape(-1, 8)[:, None, :3] + z.unsqueeze(2) * rays.reshape(-1, 8)[:, None, 3:6]).reshape(n, -1, 3).contiguous()
    with torch.no_grad():
        r_rgb, r_inv, r_sig = ref(pts)
        t_rgb, t_inv, t_sig = ref.r64(pts.double())
        q_rgb, q_inv, q_sig = nat(pts.cuda())
        d_rgb, d_inv, d_sig = nat(pts.cuda(), only_density=True)
    same = (q_inv.cpu() == r_inv.float()).squeeze(-1)
    print(f"query: {int((~same).sum())} of {same.numel()} points with a flipped frustum flag")
    assert same.float().mean().item() > 0.995
    same = same & (t_inv == r_inv).squeeze(-1)   # (and where fp64 rounding does not flip the fp32 reference's flag either)
    _close(q_rgb, r_rgb, t_rgb, same, "rgb")
    _close(q_sig, r_sig, t_sig, same, "sigma")
    assert (d_rgb == 0).all() and d_rgb.shape == q_rgb.shape
    assert torch.equal(d_sig, q_sig)


def _render(net, rays, z, n, jitter=None, lindisp=True, hard_cap=True, white=False, noise=None):
    """One composite: the fp64 twin and the fp32 reference through the composition itself, the native net through NeRFRenderer.
    ``noise`` = the unit normal draw of nerf.py:279-280 times noise_std: the kernels take it as sigma_noise, the composition draws it
    through torch.randn_like, which is pointed at the same values."""
    K = z.shape[1] if z is not None else jitter.shape[1]
    r = bts.NeRFRenderer(n_coarse=K, lindisp=lindisp, hard_alpha_cap=hard_cap, white_bkgd=white, noise_std=NOISE_STD if noise is not None else 0.0)
    if net.torch_mode:
        r.train(noise is not None)
        randn_like = torch.randn_like
        if noise is not None:
            torch.randn_like = lambda x: (noise / NOISE_STD).to(x)
        try:
            return bts.torch_modes.composite(r, net, rays, z, coarse=True, sb=n)
        finally:
            torch.randn_like = randn_like
    r.eval()
    sn = None if noise is None else noise.to(rays.device)
    if z is None:
        return r._composite(net, rays, None, True, n, True, True, True, True, False, sigma_noise=sn, jitter=jitter, want_z=True)
    return r.composite(net, rays, z, coarse=True, sb=n, sigma_noise=sn)


NOISE_STD = 0.5
# (K, hard_alpha_cap, white_bkgd, density noise, feat_shift, in-kernel sampling): the plain case, then one branch of the kernels each;
# K = 48 leaves 16 lanes of every work-group idle (5 rays of 48 samples), the re10k shape
OPTIONS = [(16, True, False, False, 0, False), (48, True, False, False, 0, False), (16, False, False, False, 0, False),
           (16, True, True, False, 0, False), (16, True, False, True, 0, False), (16, True, False, False, 1, False),
           (16, True, False, False, 0, True),
           # K = 96: R = 2 rays per work-group iteration (64 lanes idle) and more iterations than the backward's persistent grid has
           # work-groups (824 rays: 412 iterations on a grid of 208), so that pass A's loop runs twice in nearly every one
           (96, True, False, False, 0, False)]


@pytest.mark.parametrize("opt", OPTIONS, ids=["plain", "K48", "nocap", "white", "noise", "feat_shift1", "jitter", "K96"])
@pytest.mark.parametrize("shape", SHAPES, ids=["64_64_0", "32_32_1"])
def test_render_and_gradients_vs_composition(shape, opt):
    K, hard_cap, white, noisy, fs, jit = opt
    ref, nat, rays, cfg, g = _nets(*shape, fs=fs)
    n = rays.shape[0]
    rays = rays.reshape(-1, 8)
    if K > 64:   # the second iteration this case is for: render_grid has a work-group per 4 rays, rounded up to 8
        B = rays.shape[0]
        groups, grid = -(-B // (256 // K)), -(-(-(-B // 4)) // 8) * 8
        assert groups > max(8, -(-B // 4)) and groups > grid, (B, groups, grid)
    u = torch.rand(rays.shape[0], K, generator=g)
    noise = torch.randn(rays.shape[0], K, generator=g) * NOISE_STD if noisy else None
    kw = dict(hard_cap=hard_cap, white=white, noise=noise)
    if jit:   # sample_coarse inside the kernel, then the backward on the depths it hands back
        w_n, rgb_n, dep_n, a_n, inv_n, z_n, rs_n = _render(nat, rays.cuda(), None, n, jitter=u.cuda(), **kw)
        z = z_n.detach().cpu()
        assert torch.equal(z_n, bts.native.sample_coarse(rays.cuda(), u.cuda(), True))
    else:
        z = O.sample_coarse(rays, K, True, u)
        w_n, rgb_n, dep_n, a_n, inv_n, _, rs_n = _render(nat, rays.cuda(), z.cuda(), n, **kw)
    w_r, rgb_r, dep_r, a_r, inv_r, _, rs_r = _render(ref, rays, z, n, **kw)
    w_t, rgb_t, dep_t, a_t, inv_t, _, rs_t = _render(ref.r64, rays.double(), z.double(), n, **kw)
    assert rgb_n.shape == (rays.shape[0], 3) and inv_n.shape == (rays.shape[0], K, 1) and rs_n.shape == (rays.shape[0], K, 3)
    ok = (inv_n.cpu() == inv_r.float()).all(-1).all(-1)
    print(f"render {opt}: {int((~ok).sum())} of {ok.numel()} rays set aside (flipped frustum flag)")
    assert ok.float().mean().item() > 0.95
    ok = ok & (inv_t == inv_r).all(-1).all(-1)
    rel = ((dep_n.detach().cpu().double() - dep_r.detach()).abs() / dep_r.detach().abs().clamp_min(1e-6))[ok].max().item()
    print(f"  depth: max rel err {rel:.2e}")
    assert rel < 1e-4, rel
    for a, b, c, name in ((rgb_n, rgb_r, rgb_t, "rgb"), (w_n, w_r, w_t, "weights"), (a_n, a_r, a_t, "alphas"), (rs_n, rs_r, rs_t, "rgb_samps")):
        _close(a, b, c, ok, name)
    # the dead-density samples this case is built to contain: a visible share (relu(o0) == 0 in the fp64 evaluation)
    with torch.no_grad():
        pts = (rays[:, None, :3] + z.unsqueeze(2) * rays[:, None, 3:6]).reshape(n, -1, 3)
        _, _, sig = ref.r64(pts.double())
    dead = (sig == 0).float().mean().item()
    print(f"  dead-density share {dead:.2f}")
    assert dead >= 0.10
    # gradients of a seeded scalar through everything the field owns
    g_rgb, g_dep = torch.randn(rgb_r.shape, generator=g), torch.randn(dep_r.shape, generator=g) * 0.1
    # rays whose frustum flags differ between the three evaluations take another feature (learn_empty) or density (empty_empty) by a
    # finite amount: no upstream gradient on them, so that the three gradients are those of one and the same function
    g_rgb[~ok], g_dep[~ok] = 0.0, 0.0
    names = [k for k, _ in ref.mlp_coarse.named_parameters()] + [f"feats{fs}"] + (["empty"] if ref.learn_empty else [])

    def params(net):
        return list(net.mlp_coarse.parameters()) + [net.encoder.feats[fs]] + ([net.empty_feature] if net.learn_empty else [])
    gr = torch.autograd.grad((rgb_r * g_rgb).sum() + (dep_r * g_dep).sum(), params(ref), allow_unused=True)
    gt = torch.autograd.grad((rgb_t * g_rgb.double()).sum() + (dep_t * g_dep.double()).sum(), params(ref.r64), allow_unused=True)
    gn = torch.autograd.grad((rgb_n * g_rgb.cuda()).sum() + (dep_n * g_dep.cuda()).sum(), params(nat), allow_unused=True)
    for name, a, b, c in zip(names, gn, gr, gt):
        _check_grad(a, b, c, "d" + name)


def _check_grad(a, b, c, name):
    """tests/test_gpu_fused_anchor.py::_check_grads: within 1e-4 of the largest fp32 entry, or no further from fp64 than the fp32
    composition is (x 1.5 + 2e-5, max-norm and L2)."""
    scale = b.abs().max().item()
    err = (a.detach().cpu().double() - c.detach().double()).abs().max().item()
    print(f"  {name}: max err vs fp64 {err:.2e} of max |g| {scale:.2e}")
    assert scale > 0, name
    if err > 1e-4 * scale:
        _close(a, b, c, None, name, slack=2e-5)


@pytest.mark.parametrize("shape", SHAPES)
def test_dead_density_samples_still_reach_the_feature_map(shape):
    """A sample with o0 < 0 has no density gradient but a colour gradient: its texels must receive it (a liveness slot holding
    dL/do0 alone would skip them)."""
    ref, nat, rays, cfg, g = _nets(*shape)
    with torch.no_grad():
        nat.mlp_coarse.lin_out.bias[0] = -1e3     # every density dead: only the colours carry gradient
        ref.mlp_coarse.lin_out.bias[0] = -1e3
    nat.mlp_coarse.invalidate_packed(), ref.mlp_coarse.invalidate_packed()
    n, K = rays.shape[0], 16
    rays = rays.reshape(-1, 8)
    z = O.sample_coarse(rays, K, True, torch.rand(rays.shape[0], K, generator=g))
    _, rgb_r, _, _, inv_r, _, _ = _render(ref, rays, z, n)
    _, rgb_n, _, _, inv_n, _, _ = _render(nat, rays.cuda(), z.cuda(), n)
    ok = (inv_n.cpu() == inv_r).all(-1).all(-1).float().unsqueeze(-1)   # (rays with a flipped flag carry no gradient, as above)
    gf_r, = torch.autograd.grad((rgb_r * ok).sum(), [ref.encoder.feats[0]])
    gf_n, = torch.autograd.grad((rgb_n * ok.cuda()).sum(), [nat.encoder.feats[0]])
    rel = (gf_n.cpu().double() - gf_r).norm().item() / gf_r.norm().item()
    print(f"  dead densities: dF L2 rel err {rel:.2e}, max |dF| {gf_n.abs().max().item():.2e} vs {gf_r.abs().max().item():.2e}")
    assert gf_r.abs().max().item() > 0
    assert gf_n.abs().max().item() > 0.5 * gf_r.abs().max().item()
    assert rel <= 1e-4


def test_in_kernel_sampling_and_determinism():
    ref, nat, rays, cfg, g = _nets(*SHAPES[0])
    n, K = rays.shape[0], 64
    rays = rays.reshape(-1, 8).cuda()
    jit = torch.rand((rays.shape[0], K), generator=g).cuda()
    with torch.no_grad():
        a = _render(nat, rays, None, n, jitter=jit)
        z = a[5]
        b = _render(nat, rays, z, n)
        c = _render(nat, rays, z, n)
    for i in (0, 1, 2, 3, 4, 6):
        assert torch.equal(a[i], b[i]), i
        assert torch.equal(b[i], c[i]), i
    assert torch.equal(z, bts.native.sample_coarse(rays, jit, True))


def test_lean_training_path_and_fused_paths_refuse_the_mode():
    ref, nat, rays, cfg, g = _nets(*SHAPES[0])
    nat.train()
    r = bts.NeRFRenderer(n_coarse=16, lindisp=True, hard_alpha_cap=True, lean_training_outputs=True).cuda().train()
    out = r(nat, rays.cuda(), want_weights=True)
    # (no per-ray invalid sums for this head: the lean path is not taken, the full per-sample outputs come back)
    assert "weights" in out["coarse"] and "invalid_wsum" not in out["coarse"]
    with pytest.raises(bts.native.BtsNativeError, match="sample_color=False"):
        nat.occupancy_profile(torch.zeros((rays.shape[0], 64, 3), device="cuda"), 8)
