"""Novel-view frames and colour-mapped depth on the GPU (csrc/bts_frames.hip, behindthescenes_amd/novel_views.py) against the golden
fixture the reference wrote (tests/golden/novel_views.npz: its own color_tensor with matplotlib, its own render_poses and the frame
statements of gen_vid_nvs.py on CPU tensors) and, end to end, against the entry-by-entry HIP sequence with the same jitter.

Everything is compared exactly: bytes with array_equal, float64 colours and masked floats bit for bit (the kernels do the same fp32 /
fp64 operations as numpy and torch, with IEEE division).  End to end a pixel would be set aside only if its fp64 sum_k invalid *
weights lay within 1e-5 of the 0.8 threshold (the fused call's sum comes from the render epilogue, in another order); the scene is
checked on the CPU with oracle.bts_oracle's composite to hold no pixel within 1e-4 of it, and the test asserts that nothing is set aside."""
import os

import numpy as np
import pytest
import torch

import behindthescenes_amd as bts
from behindthescenes_amd import native, novel_views as NV
from oracle import bts_oracle as O

from tests import _novel_views_oracle as NO
from tests._hip_helpers import build_net

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "novel_views.npz")
DEV = "cuda:0"
K = 64
NEAR_FAR = [(3.0, 80.0), (2.5, 60.0), (3.5, 70.0)]
D_RANGE = ([3.0, 2.5, 3.5], [80.0, 60.0, 70.0])


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def cpu(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("case", ["s", "a", "b", "c", "k", "m"])      # 1 x 1, 7 x 9, 16 x 64, 33 x 70, constant, three images
def test_colour_map_against_the_golden(gold, case):
    x = torch.from_numpy(gold[f"col_{case}_x"]).to(DEV)
    imgs = x if x.dim() == 3 else x[None]
    B, h, w = imgs.shape
    for name in ("magma", "plasma", "extremes"):
        for norm in (0, 1):
            key = f"col_{case}_{name}_{norm}"
            if key + "_f64" not in gold:
                continue
            lut = gold[f"lut_{name}"]
            want64, want8 = gold[key + "_f64"].reshape(B, h, w, 3), gold[key + "_u8"].reshape(B, h, w, 3)
            N, lut_d, lut_u8 = NV._device_table(lut, x.device)
            got64 = cpu(native.colorize(imgs, N, lut_f64=lut_d, norm=bool(norm)))            # B images, min / max per image
            canvas = torch.zeros((B, h, w, 3), device=DEV, dtype=torch.uint8)
            NV.colorize_u8(imgs, lut, bool(norm), canvas)
            got8 = cpu(canvas)
            print(f"{key}: float64 values differing {int((got64 != want64).sum())}, bytes differing {int((got8 != want8).sum())}")
            assert got64.dtype == np.float64 and same_bits(got64, want64), key
            assert np.array_equal(got8, want8), key
            if B == 1:
                ct = NV.color_tensor(x, lut, norm=bool(norm))                                  # the reference's signature
                assert ct.dtype == torch.float64 and ct.device == x.device and tuple(ct.shape) == tuple(x.shape) + (3,)
                assert same_bits(cpu(ct), gold[key + "_f64"]), key


def test_colour_map_by_name_is_matplotlibs_table(gold):
    pytest.importorskip("matplotlib")
    x = torch.from_numpy(gold["col_b_x"]).to(DEV)
    N, lut, _ = NV.cmap_table("magma")
    assert same_bits(cpu(bts.color_tensor(x, "magma")), NO.colorize(gold["col_b_x"], lut))
    assert same_bits(cpu(bts.color_tensor(x, "magma", norm=True)), NO.colorize(gold["col_b_x"], lut, norm=True))


def test_canvas_placement_leaves_every_other_byte_zero(gold):
    x = gold["col_c_x"]                                                    # 33 x 70
    h, w = x.shape
    lut = gold["lut_plasma"]
    canvas = torch.zeros((2, 50, 97, 3), device=DEV, dtype=torch.uint8)
    xs = torch.from_numpy(np.stack([x, x[::-1].copy()])).to(DEV)
    NV.colorize_u8(xs, lut, False, canvas, row0=11, col0=23)
    got = cpu(canvas)
    want = np.zeros_like(got)
    want[0, 11:11 + h, 23:23 + w], want[1, 11:11 + h, 23:23 + w] = NO.colorize_u8(x, lut), NO.colorize_u8(x[::-1], lut)
    assert np.array_equal(got, want) and want.any()
    # pack_u8: a channel-planar image as x * .5 + .5, at the canvas' last rows and columns
    img = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (2, 3, 9, 13)).astype(np.float32)).to(DEV)
    canvas2 = torch.zeros((2, 20, 31, 3), device=DEV, dtype=torch.uint8)
    NV.pack_u8(img, canvas2, row0=11, col0=18, scale=0.5, shift=0.5, channels_first=True)
    want2 = np.zeros((2, 20, 31, 3), dtype=np.uint8)
    want2[:, 11:, 18:] = NO.to_u8((cpu(img) * np.float32(0.5) + np.float32(0.5)).transpose(0, 2, 3, 1))
    assert np.array_equal(cpu(canvas2), want2)
    with pytest.raises(bts.BtsNativeError):
        NV.pack_u8(img, canvas2, row0=12, col0=18, channels_first=True)    # one row too low


@pytest.mark.parametrize("case,black_invalid", [("p", 0), ("p", 1), ("q", 0), ("q", 1)])      # 5 x 7 and 24 x 40
def test_finish_kernel_on_the_golden_inputs(gold, case, black_invalid):
    rgb, depth, wsum = (torch.from_numpy(gold[f"fin_{case}_{k}"].copy())[None].to(DEV) for k in ("rgb", "depth", "wsum"))
    d_min, d_max = (float(v) for v in gold[f"fin_{case}_range"])
    canvas = NV.finish_views(rgb, depth, wsum, d_min, d_max, gold["lut_magma"], bool(black_invalid))
    got, want = cpu(canvas)[0], gold[f"fin_{case}_{black_invalid}_canvas"]
    print(f"{case} black_invalid={black_invalid}: bytes differing {int((got != want).sum())} of {want.size}")
    assert np.array_equal(got, want)
    # the masked floats, written back in place
    assert same_bits(cpu(rgb)[0], gold[f"fin_{case}_{black_invalid}_rgb"]) and same_bits(cpu(depth)[0], gold[f"fin_{case}_{black_invalid}_depth"])
    if case == "p" and black_invalid:      # the frame's maximum sat on an invalid pixel and every invalid pixel now carries it
        inv = gold["fin_p_wsum"] > np.float32(0.8)
        assert (cpu(depth)[0][inv] == gold["fin_p_depth"].max()).all() and inv.reshape(-1)[gold["fin_p_depth"].argmax()]


def test_finish_panels_at_offsets_and_two_poses_with_their_own_ranges(gold):
    g = {k: gold[f"fin_q_{k}"] for k in ("rgb", "depth", "wsum")}
    h, w = g["depth"].shape
    rgb = torch.from_numpy(np.stack([g["rgb"], g["rgb"][::-1].copy()])).to(DEV)
    depth = torch.from_numpy(np.stack([g["depth"], g["depth"][::-1].copy()])).to(DEV)
    wsum = torch.from_numpy(np.stack([g["wsum"], g["wsum"][::-1].copy()])).to(DEV)
    canvas = torch.zeros((2, h + 9, 2 * w + 5, 3), device=DEV, dtype=torch.uint8)
    NV.finish_views(rgb, depth, wsum, [2.5, 4.0], [51.3, 30.0], gold["lut_magma"], True, canvas, ((2, 1), (9, w + 5)))
    want = np.zeros((2, h + 9, 2 * w + 5, 3), dtype=np.uint8)
    for p, (lo, hi) in enumerate(((2.5, 51.3), (4.0, 30.0))):
        sl = slice(None) if p == 0 else slice(None, None, -1)
        o = NO.finish(g["rgb"][sl], g["depth"][sl], g["wsum"][sl], lo, hi, gold["lut_magma"], True)
        want[p, 2:2 + h, 1:1 + w], want[p, 9:9 + h, w + 5:] = o["img_u8"], o["depth_u8"]
    assert np.array_equal(cpu(canvas), want)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _poses():
    return torch.stack([O._pose(), O._pose(tx=0.4, ty=-0.1, tz=0.8), O._pose(tx=-0.3, tz=0.2, yaw_deg=25.0)])      # encoder, translated, rotated


@pytest.fixture(scope="module")
def field():
    cfg = O.FieldConfig()
    scene = O.synthetic_scene(1, 1, 32, 64, 64, seed=0, smooth=True)
    mlp = O.init_mlp(64 + 39, 64, 0, gen=torch.Generator().manual_seed(0))
    net = build_net(cfg, mlp, scene, [0], device=DEV)
    net.set_scale(0)
    return dict(cfg=cfg, scene=scene, mlp=mlp, net=net, st=O.make_state(scene, [0], cfg))


def _jitter(h, w):
    return torch.rand(3 * h * w, K, generator=torch.Generator().manual_seed(1000 + h))


def _renderer():
    return bts.NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True).to(DEV).eval()


_REF = {}


def reference_frames(field, h, w):
    """The entry-by-entry HIP sequence per pose -- ImageRaySampler(norm_dir=False).sample, wrapped(rays, want_weights, want_alphas) with the
    shared jitter through the renderer's sample_coarse hook, the oracle's finish -- and the CPU oracle's check of the threshold margin.
    Computed once per size and left unchanged."""
    if (h, w) in _REF:
        return _REF[(h, w)]
    poses, projs, u = _poses(), field["scene"]["projs"][:, :1], _jitter(h, w)
    r = _renderer()
    wrapped = r.bind_parallel(field["net"])
    out = dict(rgb=[], depth=[], img=[], dep=[], invalid=[], rgb_masked=[], depth_masked=[])
    aside = 0
    for p in range(3):
        up = u[p * h * w:(p + 1) * h * w]
        # the reference on the CPU: no pixel within 1e-4 of the threshold
        rays_o = O.image_rays(poses[p].view(1, 1, 4, 4), projs, h, w, *NEAR_FAR[p], norm_dir=False).reshape(-1, 8)
        with torch.no_grad():
            wts, _, _, _, inv, *_ = O.composite(rays_o, O.sample_coarse(rays_o, K, True, up), 1, field["st"], field["mlp"], field["cfg"],
                                                hard_alpha_cap=True)
        margin = ((inv[..., 0].double() * wts.double()).sum(-1) - 0.8).abs().min().item()
        print(f"{h} x {w} pose {p}: oracle's smallest distance to the 0.8 threshold {margin:.3e}")
        assert margin > 1e-4
        smp = bts.ImageRaySampler(*NEAR_FAR[p], h, w, norm_dir=False)
        rays, _ = smp.sample(None, poses[p].view(1, 1, 4, 4).to(DEV), projs.to(DEV))
        up_d = up.to(DEV)
        r.sample_coarse = lambda rr, up_d=up_d: bts.NeRFRenderer.sample_coarse(r, rr, up_d)      # the same jitter, through the renderer's hook
        with torch.no_grad():
            rd = wrapped(rays, want_weights=True, want_alphas=True)
        rd["fine"] = dict(rd["coarse"])
        c = smp.reconstruct(rd)["coarse"]
        rgb, depth = c["rgb"][0, 0, :, :, 0], c["depth"][0, 0]
        ws64 = (c["invalid"][0, 0, ..., 0].double() * c["weights"][0, 0].double()).sum(-1)
        aside += int(((ws64 - 0.8).abs() <= 1e-5).sum())
        o = NO.finish(cpu(rgb), cpu(depth), cpu(ws64).astype(np.float32), D_RANGE[0][p], D_RANGE[1][p], NV.cmap_table("magma")[1], True)
        o0 = NO.finish(cpu(rgb), cpu(depth), cpu(ws64).astype(np.float32), D_RANGE[0][p], D_RANGE[1][p], NV.cmap_table("magma")[1], False)
        out["rgb"].append(rgb.clone()), out["depth"].append(depth.clone()), out["invalid"].append(o["invalid"])
        out["img"].append((o0["img_u8"], o["img_u8"])), out["dep"].append((o0["depth_u8"], o["depth_u8"]))
        out["rgb_masked"].append(o["rgb"]), out["depth_masked"].append(o["depth"])
    out["aside"] = aside
    _REF[(h, w)] = out
    return out


def _fused(field, h, w, poses_per_call=8):
    smp = bts.ImageRaySampler(3.0, 80.0, h, w, norm_dir=False)
    return bts.FusedNovelViews(_renderer().bind_parallel(field["net"]), smp, cmap="magma", poses_per_call=poses_per_call)


@pytest.mark.parametrize("size", [(16, 32), (32, 64)])
def test_frames_against_the_entry_by_entry_sequence(field, size):
    pytest.importorskip("matplotlib")
    h, w = size
    ref = reference_frames(field, h, w)
    assert ref["aside"] == 0                                             # nothing is set aside
    assert ref["invalid"][2].any() and (~ref["invalid"][2]).any()        # the rotated pose exercises the mask
    nv = _fused(field, h, w)
    poses, projs, u = _poses().to(DEV), field["scene"]["projs"][0, 0].to(DEV), _jitter(h, w).to(DEV)
    for bi in (0, 1):
        # the floats: same kernels, same arguments (render() hands them out unmasked without black_invalid)
        rgb = torch.empty((3, h, w, 3), device=DEV)
        depth = torch.empty((3, h, w), device=DEV)
        nf = torch.tensor(NEAR_FAR, device=DEV)
        nv.render(poses, projs.expand(3, 3, 3).contiguous(), nf, None, bool(bi), None, (None, None), u, rgb, depth)
        canvas = cpu(nv.frames(poses, projs, *D_RANGE, near_far=NEAR_FAR, black_invalid=bool(bi), jitter=u))
        assert canvas.shape == (3, 2 * h, w, 3) and canvas.dtype == np.uint8
        for p in range(3):
            if not bi:
                assert torch.equal(rgb[p], ref["rgb"][p]) and torch.equal(depth[p], ref["depth"][p]), p
            else:
                assert same_bits(cpu(rgb[p]), ref["rgb_masked"][p]) and same_bits(cpu(depth[p]), ref["depth_masked"][p]), p
            d_img, d_dep = int((canvas[p, :h] != ref["img"][p][bi]).sum()), int((canvas[p, h:] != ref["dep"][p][bi]).sum())
            print(f"{h} x {w} pose {p} black_invalid={bi}: image bytes differing {d_img}, depth bytes differing {d_dep}")
            assert d_img == 0 and d_dep == 0, (p, bi)
    # the other layouts are the same panels
    img = cpu(nv.frames(poses, projs, *D_RANGE, near_far=NEAR_FAR, layout="image", jitter=u))
    dep = cpu(nv.frames(poses, projs, *D_RANGE, near_far=NEAR_FAR, layout="depth", jitter=u))
    both = cpu(nv.frames(poses, projs, *D_RANGE, near_far=NEAR_FAR, jitter=u))
    assert np.array_equal(img, both[:, :h]) and np.array_equal(dep, both[:, h:])


def test_render_poses_is_the_one_pose_chunk(field):
    h, w = 16, 32
    ref = reference_frames(field, h, w)
    wrapped = _renderer().bind_parallel(field["net"])
    smp = bts.ImageRaySampler(*NEAR_FAR[2], h, w, norm_dir=False)
    pose, projs = _poses()[2].view(1, 1, 4, 4).to(DEV), field["scene"]["projs"][:, :1].to(DEV)
    u = _jitter(h, w)[2 * h * w:].to(DEV)
    for bi in (False, True):
        torch.manual_seed(5)
        frame, depth = bts.render_poses(wrapped, smp, pose, projs, black_invalid=bi)
        assert tuple(frame.shape) == (1, h, w, 1, 3) and tuple(depth.shape) == (h, w) and frame.is_cuda and depth.is_cuda
        torch.manual_seed(5)
        own = torch.rand((h * w, K), device=DEV)                            # render_poses' one draw
        nv = bts.FusedNovelViews(wrapped, smp, cmap="magma", poses_per_call=1)
        rgb2, depth2 = torch.empty((1, h, w, 3), device=DEV), torch.empty((1, h, w), device=DEV)
        nv.render(pose[0], projs[0], torch.tensor([NEAR_FAR[2]], device=DEV), None, bi, None, (None, None), own, rgb2, depth2)
        assert torch.equal(frame[:, :, :, 0], rgb2) and torch.equal(depth, depth2[0])
        assert frame.cpu().shape == (1, h, w, 1, 3)                         # the scripts' .cpu() still works
    # with the shared jitter the values are the entry-by-entry sequence's
    nv.render(pose[0], projs[0], torch.tensor([NEAR_FAR[2]], device=DEV), None, True, None, (None, None), u, rgb2, depth2)
    assert same_bits(cpu(rgb2[0]), ref["rgb_masked"][2]) and same_bits(cpu(depth2[0]), ref["depth_masked"][2])


def test_reruns_are_bit_identical_and_chunking_changes_nothing(field):
    pytest.importorskip("matplotlib")
    h, w = 16, 32
    poses, projs, u = _poses().to(DEV), field["scene"]["projs"][0, 0].to(DEV), _jitter(h, w).to(DEV)
    kw = dict(near_far=NEAR_FAR, black_invalid=True, jitter=u)
    a = _fused(field, h, w).frames(poses, projs, *D_RANGE, **kw)
    b = _fused(field, h, w).frames(poses, projs, *D_RANGE, **kw)
    c = _fused(field, h, w, poses_per_call=2).frames(poses, projs, *D_RANGE, **kw)      # chunks of 2 + 1 poses
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and a.any()
    # without a jitter every chunk draws its own: still a frame per pose
    d = _fused(field, h, w, poses_per_call=2).frames(poses, projs, *D_RANGE, near_far=NEAR_FAR)
    assert tuple(d.shape) == (3, 2 * h, w, 3) and d.dtype == torch.uint8


def test_outside_the_envelope_is_an_error_not_a_fallback(field):
    h, w = 16, 32
    smp = bts.ImageRaySampler(3.0, 80.0, h, w, norm_dir=False)
    poses, projs = _poses().to(DEV), field["scene"]["projs"][0, 0].to(DEV)
    fine = bts.NeRFRenderer(n_coarse=K, n_fine=8, lindisp=True, hard_alpha_cap=True).to(DEV).eval().bind_parallel(field["net"])
    with pytest.raises(bts.BtsNativeError, match="fine pass"):
        bts.FusedNovelViews(fine, smp, cmap="magma").frames(poses, projs, 3.0, 80.0)
    nv = _fused(field, h, w)
    with pytest.raises(bts.BtsNativeError, match="jitter"):
        nv.frames(poses, projs, 3.0, 80.0, jitter=torch.zeros(7, K, device=DEV))
    with pytest.raises(bts.BtsNativeError, match="canvas"):
        nv.frames(poses, projs, 3.0, 80.0, canvas=torch.zeros((3, h, w, 3), device=DEV, dtype=torch.uint8), offsets=((0, 0), (h, 0)))
