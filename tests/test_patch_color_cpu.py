"""Patch colours (``image_processor: {type: patch}``, 27-channel colour targets), host side: the image processors against the real
reference's recorded output (tests/golden/patch_color.npz), the CPU oracle of the kernels pinned against the reference, the
``native_patch_color`` key and every refusal, the ABI additions (symbols, struct layout, error codes and messages: nothing launched).
No GPU needed."""
import ast
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
from oracle import bts_oracle as O
from tests import _patch_color_oracle as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "patch_color.npz")
INVALID, UNSUPPORTED = -1, -2
P = 16          # a non-NULL, 16-byte aligned pointer that is never followed
LOSSES = (("l2", "weight_guided"), ("l1", "strict"), ("l2", "none"))
_CACHE = {}


def load(name):
    """the fixture's arrays (read once, never modified): fp64 results rebuilt from their scaled differences, the depths from the jitter"""
    if name not in _CACHE:
        z = np.load(GOLDEN)
        t = {k[len(name) + 1:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "_") and not k.endswith("_meta")}
        meta = ast.literal_eval(str(z[name + "_meta"]))
        for k in [k for k in t if k.startswith("f64_")]:
            t[k] = t[k[4:]].double() + t[k].double() / meta["diff_scale"]
        t["z"] = O.sample_coarse(t["rays"].reshape(-1, 8), meta["K"], True, t["u"].float())
        t["pick"] = torch.cat([torch.arange(meta["RS"]) + b * meta["B"] for b in range(meta["n"])])
        t["sel"] = torch.cat([torch.arange(64) + b * meta["B"] for b in range(meta["n"])])
        _CACHE[name] = (t, meta)
    return _CACHE[name]


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


# ---- the image processors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
def test_patch_processor_equals_the_reference(name):
    t, meta = load(name)
    images = t["images"].float()
    for proc in (bts.PatchProcessor(3), bts.make_image_processor({"type": "patch"}), bts.make_image_processor({"type": "Patch", "patch_size": 3})):
        assert isinstance(proc, bts.PatchProcessor) and proc.channels == 27 and proc.patch_size == 3
        out = proc(images)
        assert out.dtype == torch.float32 and torch.equal(out, t["patches"].float())
    # the identity the kernels stand on: channel (y * 3 + x) * 3 + c is the RGB frame at the clamped shift (y - 1, x - 1); 12..14 the frame
    rgb = bts.RGBProcessor()(images)
    H, W = meta["H"], meta["W"]
    ii, jj = torch.arange(H), torch.arange(W)
    for y in range(3):
        for x in range(3):
            shifted = rgb[..., (ii + y - 1).clamp(0, H - 1), :][..., (jj + x - 1).clamp(0, W - 1)]
            assert torch.equal(out[:, :, (y * 3 + x) * 3:(y * 3 + x) * 3 + 3], shifted)
    assert torch.equal(out[:, :, 12:15], rgb)


def test_make_image_processor():
    assert isinstance(bts.make_image_processor({}), bts.RGBProcessor) and bts.make_image_processor({"type": "rgb"}).channels == 3
    assert bts.make_image_processor({"type": "patch", "patch_size": 5}).channels == 75
    x = torch.rand(1, 2, 3, 4, 6) * 2 - 1
    assert torch.equal(bts.RGBProcessor()(x), x * .5 + .5)
    with pytest.raises(NotImplementedError, match="LPIPS"):
        bts.make_image_processor({"type": "perceptual"})
    with pytest.raises(NotImplementedError, match="Unsupported image processor type"):
        bts.make_image_processor({"type": "sobel"})
    with pytest.raises(RuntimeError):       # an even size fails in the reference too (the shifts no longer tile the padded frame)
        bts.PatchProcessor(2)(x)
    assert "from behindthescenes_amd.image_processor import make_image_processor" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---- the oracle against the reference -----------------------------------------------------------------------------------------------------
def _oracle_inputs(t, meta, dt=torch.float32):
    ids = meta["ids_render"]
    w2c = torch.inverse(t["poses"].to(dt))[:, ids]
    imgs = (t["images"].to(dt) * .5 + .5)[:, ids]
    return imgs, w2c, t["projs"].to(dt)[:, ids]


def _within(got, r32, r64, what):
    g, r32, r64 = got.double(), r32.double(), r64.double()
    e, e_n, e_t = (g - r32).abs().max().item(), (g - r64).abs().max().item(), (r32 - r64).abs().max().item()
    print(f"  {what}: max err vs reference {e:.2e}; vs fp64 {e_n:.2e} (fp32 reference {e_t:.2e})")
    assert e <= 1e-5 or e_n <= 1.5 * e_t + 1e-5, what


@pytest.mark.parametrize("name", ["a", "b"])
def test_oracle_is_pinned_to_the_reference(name):
    t, meta = load(name)
    imgs, w2c, Ks = _oracle_inputs(t, meta)
    rays = t["rays"].reshape(-1, 8)
    samps = PC.sample_colours(imgs, w2c, Ks, rays, t["z"])
    _within(samps[t["pick"]], t["rgb_samps"], t["f64_rgb_samps"], "rgb_samps")
    _within(PC.composite(t["weights"], samps, meta["white_bkgd"]), t["rgb"], t["f64_rgb"], "rgb")
    # in fp64 the double clamp IS grid_sample over the materialised 27-channel frames
    i64, w64, K64 = _oracle_inputs(t, meta, torch.float64)
    s64 = PC.sample_colours(i64, w64, K64, rays.double(), t["z"].double())
    assert (s64[t["pick"]] - t["f64_rgb_samps"]).abs().max().item() <= 2e-6      # (the fixture's fp64 is an fp16-rounded difference: 2^-21)
    pts = (rays.double()[:, None, :3] + t["z"].double().unsqueeze(2) * rays.double()[:, None, 3:6]).reshape(meta["n"], -1, 3)
    xy = O.project(pts, w64, K64)[0]
    frames = bts.PatchProcessor(3)(t["images"].double())[:, meta["ids_render"]]
    n, nv = frames.shape[:2]
    tap = torch.nn.functional.grid_sample(frames.reshape(n * nv, 27, meta["H"], meta["W"]), xy.reshape(n * nv, 1, -1, 2), mode="bilinear",
                                          padding_mode="border", align_corners=False).view(n, nv, 27, -1).permute(0, 3, 1, 2)
    assert (tap.reshape(s64.shape) - s64).abs().max().item() <= 1e-14
    # the mutants are different functions on this data
    for m in PC.MUTANTS[:3]:
        assert (PC.sample_colours(imgs, w2c, Ks, rays, t["z"], m) - samps).abs().max().item() > 1e-3, m
    # g_weights is the derivative of composite
    w = t["weights"].double().clone().requires_grad_(True)
    g, = torch.autograd.grad((PC.composite(w, s64, meta["white_bkgd"]) * t["gin_rgb"].double()).sum(), w)
    assert (PC.g_weights(t["gin_rgb"].double(), s64, meta["white_bkgd"]) - g).abs().max().item() <= 1e-12


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("crit,policy", LOSSES)
def test_oracle_loss_is_pinned_to_the_reference(name, crit, policy):
    t, meta = load(name)
    nv = len(meta["ids_render"])
    sel = t["sel"]
    loss, g, bad = PC.pixel_loss(t["rgb"][sel].reshape(-1, nv, 27), t["loss_gt"].reshape(-1, 27), crit, policy, t["invalid"][sel], t["weights"][sel])
    ref, ref_g = t[f"loss_{crit}_{policy}"], t[f"lossg_{crit}_{policy}"]
    # (the reference's fine dict aliases the coarse one, lambda_coarse = lambda_fine = 1: loss and gradient are twice the term's)
    assert abs(2 * loss.item() - ref[0].item()) <= 1e-5
    assert (2 * g.reshape(ref_g.shape) - ref_g).abs().max().item() <= 1e-4 * ref_g.abs().max().item()
    assert abs(bad / sel.numel() - ref[1].item()) <= 1e-6


# ---- BTSNet, the renderer's companions, the loss --------------------------------------------------------------------------------------------
def _conf(**kw):
    c = dict(z_near=3.0, z_far=80.0, inv_z=True, learn_empty=True, empty_empty=False, code_mode="z",
             code=dict(num_freqs=6, freq_factor=1.5, include_input=True), encoder=dict(type="feature_map", size=(8, 16), d_out=64, num_views=4),
             mlp_coarse=dict(type="resnet", n_blocks=0, d_hidden=64), mlp_fine=dict(type="empty"))
    c.update(kw)
    return c


def _scene():
    return O.synthetic_scene(1, 4, 8, 16, 64, seed=3, intrinsics=O.K_KITTI360, yaw_deg=9.0, smooth=True)


def test_encode_without_the_key_names_it():
    s = _scene()
    frames = bts.PatchProcessor(3)(s["images"])
    net = bts.BTSNet(_conf()).eval()
    assert not net.native_patch_color
    with pytest.raises(NotImplementedError, match="native_patch_color: true"):
        net.encode(s["images"], s["projs"], s["poses"], ids_encoder=[0], ids_render=[1, 2], images_alt=frames)
    # with the key the 27 channels are accepted (and the hand-over, HIP, says loudly that these are CPU tensors)
    net = bts.BTSNet(_conf(native_patch_color=True)).eval()
    with pytest.raises(bts.BtsNativeError, match="GPU"):
        net.encode(s["images"], s["projs"], s["poses"], ids_encoder=[0], ids_render=[1, 2], images_alt=frames)
    assert net._patch == 3
    # three and four channels keep their meaning
    assert net._patch_of(None) == 0 and net._patch_of(frames[:, :, :3]) == 0 and net._patch_of(frames[:, :, :4]) == 0


def test_encode_refusals():
    s = _scene()
    frames = bts.PatchProcessor(3)(s["images"])
    for extra in (dict(sample_color=False), dict(sample_color=False, native_mlp_color=True)):
        net = bts.BTSNet(_conf(native_patch_color=True, **extra)).eval()
        with pytest.raises(NotImplementedError, match="patch colours with sample_color: false"):
            net.encode(s["images"], s["projs"], s["poses"], ids_encoder=[0], ids_render=[1], images_alt=frames)
    for extra in (dict(), dict(native_multi_view=True)):      # the torch-composed mode and the merged-view kernels
        net = bts.BTSNet(_conf(native_patch_color=True, **extra)).eval()
        with pytest.raises(NotImplementedError, match="patch colours with merged encoder views"):
            net.encode(s["images"], s["projs"], s["poses"], ids_encoder=[0, 2], ids_render=[1], images_alt=frames)
        with pytest.raises(NotImplementedError, match="patch colours with merged encoder views"):
            net.encode(s["images"], s["projs"], s["poses"], ids_encoder=[0], ids_render=[1, 2], images_alt=frames, combine_ids=[(1, 2)])


def test_fused_paths_name_patch_colours():
    net = bts.BTSNet(_conf(native_patch_color=True)).train()
    renderer = bts.NeRFRenderer.from_conf(dict(n_coarse=64, lindisp=True, hard_alpha_cap=True, lean_training_outputs=True)).train()
    crit = bts.ReconstructionLoss({"criterion": "l1+ssim", "invalid_policy": "weight_guided"})
    msg = native.PATCH_COLOR_MESSAGE
    assert "patch colours" in msg
    sampler = bts.PatchRaySampler(ray_batch_size=256, z_near=3.0, z_far=80.0, patch_size=8, channels=27)
    assert bts.FusedTrainStep(renderer.bind_parallel(net).train(), sampler, crit).why_not(None, [0], [1], [0, 1]) == msg
    net._patch = 3        # (what encode leaves behind)
    sampler3 = bts.PatchRaySampler(ray_batch_size=256, z_near=3.0, z_far=80.0, patch_size=8)
    assert bts.FusedTrainStep(renderer.bind_parallel(net).train(), sampler3, crit).why_not(None, [0], [1], [0, 1]) == msg
    net.eval(), renderer.eval()
    assert bts.FusedEvalFrame(renderer.bind_parallel(net).eval(), bts.ImageRaySampler(3.0, 80.0, 8, 16)).why_not(None, [0], [0]) == msg
    assert bts.FusedEvalFrame(renderer.bind_parallel(net).eval(), bts.ImageRaySampler(3.0, 80.0, 8, 16, channels=27)).why_not(None, [0], [0]) == msg
    from behindthescenes_amd import novel_views
    assert novel_views._why_not(renderer.bind_parallel(net).eval(), bts.ImageRaySampler(3.0, 80.0, 8, 16)) == msg
    # the sparse one-shot projection of the lean training render
    net._has_latents, net._latents_ms = True, [torch.zeros(1, 1, 64, 8, 16)]
    with pytest.raises(bts.BtsNativeError, match="patch colours"):
        net.native_field(sampled=(torch.zeros(4, 8), None, torch.zeros(4, 64), True))
    net.invalidate_field_state()
    assert net._patch == 0


def _loss_data(c=27, nv=2, K=4):
    g = torch.Generator().manual_seed(5)
    level = dict(rgb=torch.rand(1, 1, 8, 8, nv, c, generator=g), depth=torch.rand(1, 1, 8, 8, generator=g) + 3,
                 weights=torch.rand(1, 1, 8, 8, K, generator=g), invalid=torch.zeros(1, 1, 8, 8, K, nv),
                 rgb_samps=torch.rand(1, 1, 8, 8, K, nv * c, generator=g))
    return dict(coarse=[level], fine=[dict(level)], rgb_gt=torch.rand(1, 1, 8, 8, c, generator=g))


@pytest.mark.parametrize("conf,word", [
    (dict(criterion="l1+ssim", invalid_policy="strict"), r"criterion 'l1\+ssim' on 27 colour channels"),
    (dict(criterion="l2", invalid_policy="strict", median_thresholding=True, native_pixel_loss=True), "median_thresholding on 27"),
    (dict(criterion="l1", invalid_policy="weight_guided_diverse", native_pixel_loss=True), "weight_guided_diverse"),
    (dict(criterion="l2", invalid_policy="strict", lambda_edge_aware_smoothness=0.001, native_pixel_loss=True), "lambda_edge_aware_smoothness > 0"),
])
def test_loss_options_deferred_on_27_channels_name_themselves(conf, word):
    with pytest.raises(NotImplementedError, match=word):
        bts.ReconstructionLoss(conf)(_loss_data())


def test_automasking_on_other_than_3_channels_names_itself():
    crit = bts.ReconstructionLoss(dict(criterion="l2", invalid_policy="strict", native_pixel_loss=True, native_automask=True), use_automasking=True)
    data = _loss_data()
    data["rgb_gt"] = torch.rand(1, 1, 8, 8, 4)     # (the colours and the error map: the rendered rgb keeps its 27)
    with pytest.raises(NotImplementedError, match="use_automasking on 27"):
        crit(data)


def test_pixel_loss_channels_rejects_what_it_does_not_serve():
    x = torch.zeros(4, 54)
    with pytest.raises(bts.BtsNativeError, match="criterion"):
        native.pixel_loss_channels(x, torch.zeros(4, 27), None, None, "l1+ssim", "none")
    with pytest.raises(bts.BtsNativeError, match="none / strict / weight_guided"):
        native.pixel_loss_channels(x, torch.zeros(4, 27), None, None, "l2", "weight_guided_diverse")


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("bts_patch_color_fwd", "bts_patch_color_bwd", "bts_patch_color_query", "bts_pixel_loss_channels_workspace", "bts_pixel_loss_channels")


def test_symbols_are_exported_and_the_abi_is_still_9(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.bts_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert _lib.BTS_PATCH_COLOR_SIZE == 3 and _lib.BTS_PATCH_COLOR_CHANNELS == 27


def test_ctypes_struct_matches_the_c_layout():
    fields = [f for f, _ in _lib.BtsPatchColor._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "bts_render.h"\nint main(void) {\n  printf("%zu\\n", sizeof(BtsPatchColor));\n' + \
        "".join(f'  printf("%zu\\n", offsetof(BtsPatchColor, {f}));\n' for f in fields) + \
        '  printf("%d %d %d\\n", BTS_PATCH_COLOR_SIZE, BTS_PATCH_COLOR_CHANNELS, BTS_PIXEL_LOSS_MAX_CHANNELS);\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == C.sizeof(_lib.BtsPatchColor)
    assert [int(x) for x in out[1:1 + len(fields)]] == [getattr(_lib.BtsPatchColor, f).offset for f in fields]
    assert [int(x) for x in out[1 + len(fields):]] == [3, 27, native.PIXEL_LOSS_MAX_CHANNELS]


def _pc(**kw):
    base = dict(n=2, nv=3, H=16, W=32, K=16, patch=3, white_bkgd=0, reserved_=0, rays_per_sample=90, rays=P, z_samp=P, weights=P, imgs_nhwc4=P,
                K_r=P, w2c_r=P, rgb=P, rgb_samps=None)
    base.update(kw)
    return _lib.BtsPatchColor(**base)


def _call(lib, entry, a, *rest):
    fn = getattr(lib, entry)
    if entry == "bts_patch_color_fwd":
        return fn(None if a is None else C.byref(a), None)
    if entry == "bts_patch_color_bwd":
        g_rgb, g_w = rest if rest else (P, P)
        return fn(None if a is None else C.byref(a), g_rgb, g_w, None)
    xyz, n_pts, rgb = rest if rest else (P, 8, P)
    return fn(None if a is None else C.byref(a), xyz, n_pts, rgb, None)


ENTRIES = ("bts_patch_color_fwd", "bts_patch_color_bwd", "bts_patch_color_query")


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_checks_shared_by_the_three(lib, entry):
    def err():
        return lib.bts_last_error().decode()
    assert _call(lib, entry, None) == INVALID and err() == f"{entry}: NULL argument struct"
    for f in ("imgs_nhwc4", "K_r", "w2c_r"):
        assert _call(lib, entry, _pc(**{f: None})) == INVALID and "NULL pointer among imgs_nhwc4, K_r, w2c_r" in err()
    assert _call(lib, entry, _pc(imgs_nhwc4=24)) == INVALID and "imgs_nhwc4 needs 16 bytes" in err()
    assert _call(lib, entry, _pc(K_r=18)) == INVALID and "misaligned" in err()
    for f in ("n", "nv", "H", "W"):
        assert _call(lib, entry, _pc(**{f: 0})) == INVALID and "non-positive size" in err()
    assert _call(lib, entry, _pc(nv=9)) == INVALID and "BTS_MAX_VIEWS" in err()
    for size in (1, 2, 5, 0):
        assert _call(lib, entry, _pc(patch=size)) == UNSUPPORTED
        assert err() == f"{entry}: patch={size}, but the compiled patch size is 3 (27 channels)"
    if entry != "bts_patch_color_query":      # (the query reads neither: test_entry_checks_of_each)
        for f in ("rays", "z_samp"):
            assert _call(lib, entry, _pc(**{f: None})) == INVALID and "NULL pointer" in err()
        for f in ("K", "rays_per_sample"):
            assert _call(lib, entry, _pc(**{f: 0})) == INVALID and "non-positive size" in err()
        assert _call(lib, entry, _pc(rays=18)) == INVALID and "misaligned" in err()
        assert _call(lib, entry, _pc(n=1 << 20, rays_per_sample=1 << 20)) == UNSUPPORTED and "too many rays or points" in err()


def test_entry_checks_of_each(lib):
    def err():
        return lib.bts_last_error().decode()
    assert _call(lib, "bts_patch_color_fwd", _pc(weights=None)) == INVALID and err() == "bts_patch_color_fwd: NULL pointer among weights, rgb"
    assert _call(lib, "bts_patch_color_fwd", _pc(rgb=None)) == INVALID and "weights, rgb" in err()
    assert _call(lib, "bts_patch_color_fwd", _pc(rgb_samps=18)) == INVALID and "rgb_samps" in err()
    assert _call(lib, "bts_patch_color_bwd", _pc(), None, P) == INVALID and err() == "bts_patch_color_bwd: NULL pointer among g_rgb, g_weights"
    assert _call(lib, "bts_patch_color_bwd", _pc(), P, None) == INVALID
    assert _call(lib, "bts_patch_color_bwd", _pc(), P, 18) == INVALID and "misaligned" in err()
    assert _call(lib, "bts_patch_color_query", _pc(), None, 8, P) == INVALID and err() == "bts_patch_color_query: NULL pointer among xyz, rgb"
    assert _call(lib, "bts_patch_color_query", _pc(), P, 0, P) == INVALID and "P=0" in err()
    # the query reads neither rays nor K
    assert _call(lib, "bts_patch_color_query", _pc(rays=None, z_samp=None, K=0, rays_per_sample=0), P, 0, P) == INVALID and "P=0" in err()


def _px(**kw):
    base = dict(rgb=P, rgb_gt=P, out=P, B=128, n=1, patch_h=1, patch_w=1, nv=2, K=0, criterion=2, invalid_policy=0, scale_rgb=1.0)
    base.update(kw)
    return _lib.BtsPixelLossArgs(**base)


def test_pixel_loss_channels_entry_checks(lib):
    who = "bts_pixel_loss_channels"

    def call(a, ch=27, ws=P, ws_bytes=1 << 20):
        return lib.bts_pixel_loss_channels(None if a is None else C.byref(a), ch, ws, ws_bytes, None), lib.bts_last_error().decode()
    assert call(None) == (INVALID, f"{who}: NULL required pointer (args, rgb, rgb_gt, out)")
    for f in ("rgb", "rgb_gt", "out"):
        assert call(_px(**{f: None}))[0] == INVALID
    assert call(_px(B=0)) == (INVALID, f"{who}: non-positive size (B, nv)")
    assert call(_px(nv=0))[0] == INVALID
    assert call(_px(B=(1 << 29) + 1)) == (INVALID, f"{who}: {(1 << 29) + 1} rays are more than 2^29")
    for ch in (0, 28, -1):
        assert call(_px(), ch) == (INVALID, f"{who}: {ch} channels are outside [1, 27]")
    assert call(_px(criterion=3))[0] == INVALID and call(_px(invalid_policy=4))[0] == INVALID
    for kw in (dict(median_thresholding=1), dict(invalid_policy=3), dict(edge_aware_smoothness=1)):
        rc, msg = call(_px(**kw))
        assert rc == UNSUPPORTED and "median_thresholding, weight_guided_diverse and edge_aware_smoothness" in msg
    assert call(_px(invalid_policy=1))[0] == INVALID        # strict without invalid / invalid_any
    assert call(_px(invalid_policy=2, invalid=P, K=4))[0] == INVALID      # weight_guided without weights
    need = lib.bts_pixel_loss_channels_workspace(128)
    assert need > 0 and lib.bts_pixel_loss_channels_workspace(0) == 0 and lib.bts_pixel_loss_channels_workspace((1 << 29) + 1) == 0
    assert call(_px(), ws=None)[0] == INVALID and call(_px(), ws_bytes=need - 1)[0] == INVALID
    assert "workspace too small" in call(_px(), ws_bytes=need - 1)[1]
