"""GPU: every rung of the host dispatch once -- the three compiled field shapes (C, d_hidden, n_blocks) x the four view-count rungs
(nv = 1, 2, 3, 5 -> per-view arrays of 1, 2, 4, 8; 3 and 5 are the smallest counts that need 4 and 8) x the four dispatched launches: the
render forward on the projected map, the render forward on raw channels-last features, the render backward and the field query.  A
dispatch that picks a kernel built for another shape or for fewer views computes wrong numbers without an error, so every case is held
against the CPU oracle.  One batch element, a 32 x 64 map, 128 rays; K = 64 throughout, K = 8 for (64, 64, 0) (several rays per wave
iteration) and K = 48 for (32, 32, 1) (the 48-lane forward and the 48-lane row pass of the backward).
Tolerances and masks are those of tests/test_gpu_parity.py (forward: _check; field query: the golden query test) and
tests/test_gpu_grad.py (backward: 1e-4 of each tensor's largest entry, rays near a frustum border or a relu kink get a zero upstream
gradient in both paths)."""
import pytest
import torch

from behindthescenes_amd import synthetic
from oracle import bts_oracle as O
from tests._cases import robust_ray_mask
from tests.test_gpu_grad import GRAD_RTOL, REAL_SHAPES, _gate_safe_rays, _hip_grads, _oracle_grads, _rel_to_max
from tests.test_gpu_parity import ABS_TOL, _check

pytestmark = pytest.mark.gpu

H, W, RAYS = 32, 64, 128
RE10K = dict(cfg=dict(d_min=1.0, d_max=100.0, code_mode="distance"), intr=O.K_RE10K, baseline=0.2, hard_cap=False, depth_floor=1e-3)
KITTI = dict(cfg=dict(), intr=O.K_KITTI360, baseline=0.54, hard_cap=True, depth_floor=0.0)
# (C, d_hidden, n_blocks, K)
SHAPES = [(64, 64, 0, 64), (64, 64, 0, 8), (32, 32, 1, 64), (32, 32, 1, 48), (32, 32, 0, 64)]
CASES = [s + (nv,) for s in SHAPES for nv in (1, 2, 3, 5)]
IDS = ["C%d_hd%d_nb%d_K%d_nv%d" % c for c in CASES]
MIN_KEPT = min(s["min_kept"] for s in REAL_SHAPES.values())     # the smallest fraction of rays test_gpu_grad.py accepts behind its kink mask
_CACHE = {}


def _case(C, Hd, nb, K, nv):
    """Scene, rays, masks and the oracle's outputs and gradients of one case: CPU only, computed once and shared by the four tests."""
    key = (C, Hd, nb, K, nv)
    if key in _CACHE:
        return _CACHE[key]
    s = RE10K if nb else KITTI
    cfg = O.FieldConfig(**s["cfg"])
    seed = 1000 + 10 * K + nv
    g = torch.Generator().manual_seed(seed)
    ids_render = list(range(1, nv + 1))
    scene = synthetic.synthetic_scene(1, nv + 1, H, W, C, seed=seed, intrinsics=s["intr"], baseline=s["baseline"], smooth=True)
    mlp = O.init_mlp(C + 39, Hd, nb, gen=g)
    rays = O.image_rays(scene["poses"], scene["projs"], H, W, cfg.d_min, cfg.d_max)
    rays = rays[:, torch.randperm(rays.shape[1], generator=g)[:RAYS].sort().values].contiguous()            # (1, 128, 8)
    z = O.sample_coarse(rays.reshape(-1, 8), K, True, torch.rand(RAYS, K, generator=g))
    st = O.make_state(scene, ids_render, cfg)
    robust = robust_ray_mask(st, rays, z)
    safe, _ = _gate_safe_rays(scene, mlp, cfg, ids_render, rays, z, None, margin=2e-5)
    mask = (robust & safe.view(-1)).float()
    c_rgb = torch.randn(RAYS, nv * 3, generator=g) * mask.unsqueeze(-1)

    def loss_fn(w, rgb, depth, a):
        return (rgb * c_rgb.to(rgb.device, rgb.dtype)).sum() + 0.05 * (depth * mask.to(depth.device, depth.dtype)).sum()

    with torch.no_grad():
        ow, orgb, odepth, oa, oinv, _, _ = O.composite(rays.reshape(-1, 8), z, 1, st, mlp, cfg, hard_alpha_cap=s["hard_cap"])
        pts = (rays[:, :, None, :3] + z.view(1, RAYS, K, 1) * rays[:, :, None, 3:6]).reshape(1, -1, 3).contiguous()
        q_rgb, q_inv, q_sigma = O.field_forward(pts, st, mlp, cfg)
    grads = _oracle_grads(scene, mlp, cfg, ids_render, rays, z, 1, s["hard_cap"], loss_fn)
    _CACHE[key] = dict(s=s, cfg=cfg, scene=scene, mlp=mlp, ids_render=ids_render, rays=rays, z=z, st=st, robust=robust, mask=mask,
                       loss_fn=loss_fn, fwd=dict(w=ow, rgb=orgb, depth=odepth, a=oa, inv=oinv), pts=pts, q=(q_rgb, q_inv, q_sigma),
                       grads=grads)
    return _CACHE[key]


@pytest.fixture(scope="module")
def hip():
    import behindthescenes_amd as bts
    from behindthescenes_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return bts


def _net(c, train=False):
    from tests._hip_helpers import build_net
    return build_net(c["cfg"], c["mlp"], c["scene"], c["ids_render"], train=train)


def _check_forward(c, w, rgb, depth, a, inv):
    """tests/test_gpu_parity.py's _oracle_vs_hip bookkeeping + _check on this case's rays"""
    o = c["fwd"]
    assert c["robust"].float().mean() > 0.5
    flips = (inv.cpu() != o["inv"]).any(-1).any(-1)
    assert not flips[c["robust"]].any(), "invalid flag differs on a ray that keeps a 1e-4 margin from every frustum border"
    r = dict(depth=(depth.cpu(), o["depth"]), rgb=(rgb.cpu(), o["rgb"]), w=(w.cpu(), o["w"]), a=(a.cpu(), o["a"]), flips=flips,
             robust=c["robust"], on_border=~robust_ray_mask(c["st"], c["rays"], c["z"], margin=3e-6))
    _check(r, depth_floor=c["s"]["depth_floor"])


@pytest.mark.parametrize("C,Hd,nb,K,nv", CASES, ids=IDS)
def test_render_forward_on_the_projected_map(hip, C, Hd, nb, K, nv):
    c = _case(C, Hd, nb, K, nv)
    renderer = hip.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=c["s"]["hard_cap"]).cuda().eval()
    with torch.no_grad():
        w, rgb, depth, a, inv, _, _ = renderer.composite(_net(c), c["rays"].reshape(-1, 8).cuda(), c["z"].cuda(), sb=1)
    assert rgb.shape == (RAYS, nv * 3) and inv.shape == (RAYS, K, nv)
    _check_forward(c, w, rgb, depth, a, inv)


@pytest.mark.parametrize("C,Hd,nb,K,nv", CASES, ids=IDS)
def test_render_forward_on_raw_features(hip, C, Hd, nb, K, nv):
    from behindthescenes_amd import native
    c = _case(C, Hd, nb, K, nv)
    net = _net(c)
    with torch.no_grad():
        ft = net.native_field()
        feat_nhwc = native.nchw_to_nhwc(net.grid_f_features[0][:, 0].detach().contiguous())
        ftd = native.FieldTensors(net.spec, None, ft.K_enc, ft.w2c_enc, ft.imgs_nhwc4, ft.K_r, ft.w2c_r, ft.empty_feature, feat_nhwc=feat_nhwc)
        o = native.render_fwd(ftd, net.mlp_coarse.packed().detach(), c["rays"].reshape(-1, 8).cuda(), c["z"].cuda(),
                              hard_alpha_cap=c["s"]["hard_cap"], want_weights=True, want_alphas=True)
    assert o["rgb"].shape == (RAYS, nv * 3) and o["invalid"].shape == (RAYS, K, nv)
    _check_forward(c, o["weights"], o["rgb"], o["depth"], o["alphas"], o["invalid"] > 0)


@pytest.mark.parametrize("C,Hd,nb,K,nv", CASES, ids=IDS)
def test_render_backward(hip, C, Hd, nb, K, nv):
    c = _case(C, Hd, nb, K, nv)
    kept = float(c["mask"].mean())
    assert kept > MIN_KEPT, kept
    renderer = hip.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=c["s"]["hard_cap"]).cuda()
    ours = _hip_grads(hip, _net(c, train=True), renderer, c["rays"].reshape(-1, 8).cuda(), c["z"].cuda(), 1, c["loss_fn"])
    names = ["w_in", "b_in"] + (["fc_0.w", "fc_0.b", "fc_1.w", "fc_1.b"] if nb else []) + ["w_out", "b_out", "feat"]
    assert len(ours) == len(c["grads"]) == len(names)
    errs = {nme: _rel_to_max(a, b.view_as(a.cpu())) for a, b, nme in zip(ours, c["grads"], names)}
    print(f"kept {kept:.2f}; max err / max entry: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for nme, err in errs.items():
        assert err <= GRAD_RTOL, (nme, err)


@pytest.mark.parametrize("C,Hd,nb,K,nv", CASES, ids=IDS)
def test_field_query(hip, C, Hd, nb, K, nv):
    c = _case(C, Hd, nb, K, nv)
    q_rgb, q_inv, q_sigma = c["q"]
    with torch.no_grad():
        rgb, inv, sig = _net(c)(c["pts"].cuda())
    assert rgb.shape == q_rgb.shape and inv.shape == q_inv.shape and sig.shape == q_sigma.shape
    same = inv.cpu() == q_inv
    assert same.float().mean().item() > 0.995
    keep = same.all(dim=-1)
    torch.testing.assert_close(rgb.cpu()[keep], q_rgb[keep], rtol=0, atol=ABS_TOL)
    torch.testing.assert_close(sig.cpu()[keep], q_sigma[keep], rtol=1e-4, atol=1e-6)
