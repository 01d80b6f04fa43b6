"""Tensor-level access to the HIP renderer: validates torch tensors (device, dtype, contiguity, shape), hands raw
device pointers + the current HIP stream to the C ABI (include/bts_render.h) and wraps the forward/backward pair in a
``torch.autograd.Function``.  PyTorch is plumbing here (memory, streams, autograd bookkeeping); every computation of
the render path happens in libbts_render.so and nothing in this module falls back to torch ops."""
from dataclasses import dataclass
from typing import Optional

import ctypes as C
import math
import weakref

import torch

from . import _lib
from ._lib import BtsFieldCfg, BtsFieldTensors, BtsNativeError, BtsRenderArgs, BtsRenderGrads


@dataclass(frozen=True)
class FieldSpec:
    """Static shape/config of the field (mirrors BtsFieldCfg minus n/H/W/nv, which come from the tensors)."""
    C: int
    d_hidden: int
    n_blocks: int
    num_freqs: int = 6
    freq_factor: float = 1.5
    d_min: float = 3.0
    d_max: float = 80.0
    inv_z: bool = True
    code_mode: str = "z"
    learn_empty: bool = False
    empty_empty: bool = False
    # the geometry of the map's tile flags (BtsFieldCfg.tile_blocks, ABI 9): 16 x 4 blocks (True: faster with a channels-last feature map)
    # or runs of 64 texels (False: faster with an NCHW one).  Every call on one (d_proj, tiles) pair must use the same spec.
    tile_blocks: bool = False
    # MLP-predicted colour (sample_color=False, models_bts.py:41-42, 315-321): a four-output lin_out, served by the *_mlp_color entries
    mlp_color: bool = False

    @property
    def d_in(self):
        return self.C + 3 + 6 * self.num_freqs

    def mlp_param_count(self):
        hd = self.d_hidden
        d_out = 4 if self.mlp_color else 1
        return hd * self.d_in + hd + self.n_blocks * (2 * hd * hd + 2 * hd) + d_out * hd + d_out


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(t: torch.Tensor):
    """The current HIP stream of the tensor's device.  The library launches on the CURRENT device, so a tensor that lives elsewhere
    is rejected here instead of enqueuing its pointers on the wrong GPU."""
    if t.device.index is not None and t.device.index != torch.cuda.current_device():
        raise BtsNativeError(f"tensor on {t.device} but the current device is cuda:{torch.cuda.current_device()}: wrap the call in "
                             "torch.cuda.device(...) (one process per GPU never hits this)")
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _addr(t: Optional[torch.Tensor]):
    """the device address for a pointer field of an argument struct (None: NULL)"""
    return None if t is None else t.data_ptr()


def _req_as(t, name: str, dtype, shape=None, contiguous=True):
    """THE tensor check: a GPU tensor of ``dtype``, contiguous (unless the entry point reads strides), of ``shape`` when given"""
    if not isinstance(t, torch.Tensor):
        raise BtsNativeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise BtsNativeError(f"{name}: must live on the GPU (got {t.device}); the HIP renderer has no CPU path")
    if t.dtype != dtype:
        raise BtsNativeError(f"{name}: must be {str(dtype).split('.')[-1]} (got {t.dtype})")
    if contiguous and not t.is_contiguous():
        raise BtsNativeError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise BtsNativeError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _req(t, name: str, shape=None):
    return _req_as(t, name, torch.float32, shape)


def _req_tiles(tiles, n_tiles, dev, whose):
    """the tile flags of a projected map (a ValueError, as ever)"""
    if tiles.dtype != torch.uint8 or not tiles.is_contiguous() or tiles.numel() != n_tiles or tiles.device != dev:
        raise ValueError(f"tiles: expected a contiguous uint8 tensor of (N, proj_tile_count) on {whose} device")


def _scratch(dev, n_bytes):
    """Fresh scratch of at least 16 bytes from torch's allocator (the library allocates nothing); it goes back to the caching allocator
    with the call.  (_workspace below is the kept per-stream buffer of the entry points that run every step.)"""
    return torch.empty(max(int(n_bytes), 16), device=dev, dtype=torch.uint8)


# --------------------------------------------------------------------------------------------------------------
# layout / edge kernels
# --------------------------------------------------------------------------------------------------------------
def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    """(N, C, H, W) -> (N, H, W, C) copy (bts_nchw_to_nhwc)."""
    _req(x, "x")
    N, Cc, H, W = x.shape
    out = torch.empty((N, H, W, Cc), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().bts_nchw_to_nhwc(_ptr(x), _ptr(out), N, Cc, H, W, _stream(x)), "bts_nchw_to_nhwc")
    return out


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    _req(x, "x")
    N, H, W, Cc = x.shape
    out = torch.empty((N, Cc, H, W), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().bts_nhwc_to_nchw(_ptr(x), _ptr(out), N, Cc, H, W, _stream(x)), "bts_nhwc_to_nchw")
    return out


def pack_rgb(images: torch.Tensor, scale: float = 1.0, shift: float = 0.0) -> torch.Tensor:
    """(..., 3, H, W) -> (..., H, W, 4) rgb0 with x*scale+shift (bts_pack_rgb)."""
    _req(images, "images")
    lead, (c, H, W) = images.shape[:-3], images.shape[-3:]
    if c != 3:
        raise BtsNativeError(f"images: expected 3 channels, got {c}")
    N = 1
    for d in lead:
        N *= d
    out = torch.empty(tuple(lead) + (H, W, 4), device=images.device, dtype=torch.float32)
    _lib.check(_lib.load().bts_pack_rgb(_ptr(images), _ptr(out), N, H, W, scale, shift, _stream(images)), "bts_pack_rgb")
    return out


def gen_rays(poses_c2w: torch.Tensor, projs: torch.Tensor, H: int, W: int, z_near: float, z_far: float,
             norm_dir: bool = True) -> torch.Tensor:
    """poses (V,4,4), projs (V,3,3) -> rays (V,H,W,8) (bts_gen_rays)."""
    V = poses_c2w.shape[0]
    _req(poses_c2w, "poses_c2w", (V, 4, 4)), _req(projs, "projs", (V, 3, 3))
    out = torch.empty((V, H, W, 8), device=poses_c2w.device, dtype=torch.float32)
    _lib.check(_lib.load().bts_gen_rays(_ptr(poses_c2w), _ptr(projs), V, H, W, z_near, z_far, int(norm_dir), _ptr(out),
                                        _stream(out)), "bts_gen_rays")
    return out


def patch_rays(poses_c2w, projs, images, patch_v, patch_y, patch_x, ph: int, pw: int, z_near: float, z_far: float, norm_dir: bool = True):
    """poses (n,v,4,4), projs (n,v,3,3), images (n,v,c,H,W) | None with (H, W) given via ``images`` or a (H, W) tuple; patch_* (n,P)
    int32 -> rays (n, P*ph*pw, 8), rgb_gt (n, P*ph*pw, c) | None  (bts_patch_rays)."""
    n, v = poses_c2w.shape[:2]
    _req(poses_c2w, "poses_c2w", (n, v, 4, 4)), _req(projs, "projs", (n, v, 3, 3))
    if isinstance(images, tuple):
        (H, W), c, images = images, 0, None
    else:
        _req(images, "images")
        c, H, W = images.shape[2:]
    P = patch_v.shape[1]
    if not isinstance(images, tuple) and ((ph > H) or (pw > W)):
        raise BtsNativeError(f"patch {ph}x{pw} does not fit a {H}x{W} frame")
    for t, nme in ((patch_v, "patch_v"), (patch_y, "patch_y"), (patch_x, "patch_x")):
        _req_as(t, nme, torch.int32, (n, P))
    dev = poses_c2w.device
    rays = torch.empty((n, P * ph * pw, 8), device=dev, dtype=torch.float32)
    gt = torch.empty((n, P * ph * pw, c), device=dev, dtype=torch.float32) if images is not None else None
    _lib.check(_lib.load().bts_patch_rays(_ptr(poses_c2w), _ptr(projs), _ptr(images), patch_v.data_ptr(), patch_y.data_ptr(),
                                          patch_x.data_ptr(), n, v, c, H, W, P, ph, pw, z_near, z_far, int(norm_dir), _ptr(rays),
                                          _ptr(gt), _stream(rays)), "bts_patch_rays")
    return rays, gt


PIXEL_CRITERIA = {"l1": 1, "l2": 2}
# THE invalid-ray policies (loss.py:100-118) as the kernels number them.  The l1+ssim entry points take the prefix without the diverse rule
# (its per-(ray, view) flags go in as invalid_any under strict: loss_diverse_flags)
PIXEL_POLICIES = {None: 0, "none": 0, "strict": 1, "weight_guided": 2, "weight_guided_diverse": 3}
INVALID_POLICIES = {name: p for name, p in PIXEL_POLICIES.items() if p <= 2}

WAVE_PATCH_PIXELS = 64      # bts_photometric_loss: one wave per patch, lane = pixel


def _invalid_inputs(invalid_policy, table, B, weights, invalid, invalid_wsum, invalid_any, rgb_samps=None, nv=None):
    """THE rule for which invalid-ray inputs a policy reads, for the four loss entry points: ``table`` is the policy table the entry point
    accepts, ``nv`` the number of views where the caller knows it (else it is the tensors').  The renderer's per-ray reductions
    (render_fwd(want_invalid_sums=True)) stand in for the per-sample tensors when given: invalid_wsum (B, nv) under weight_guided,
    invalid_any (B, nv) under strict.  Else strict reads invalid (B, K, nv), weight_guided weights (B, K) too, weight_guided_diverse
    rgb_samps (B, K, nv, 3) too (and never the sums).
    -> (policy number, K of the per-sample tensors | 0, nv | 0, {name: tensor | None} of the five, None where the policy does not read it)"""
    policy = table[invalid_policy]
    masks = dict(weights=None, invalid=None, invalid_wsum=None, invalid_any=None, rgb_samps=None)
    K = 0
    sums = invalid_wsum if policy == 2 else invalid_any if policy == 1 else None
    if sums is not None:
        nv = sums.shape[-1] if nv is None else nv
        masks["invalid_wsum" if policy == 2 else "invalid_any"] = _req(sums, "invalid_wsum / invalid_any", (B, nv))
    elif policy:
        if nv is None:
            _req(invalid, "invalid")
            nv = invalid.shape[2]
        K = invalid.shape[1]
        masks["invalid"] = _req(invalid, "invalid", (B, K, nv))
        if policy >= 2:
            masks["weights"] = _req(weights, "weights", (B, K))
        if policy == 3:
            masks["rgb_samps"] = _req(rgb_samps, "rgb_samps", (B, K, nv, 3))
    return policy, K, nv or 0, masks


def _rgb_loss_inputs(rgb, depth, rgb_gt, thresh, eas, invalid_policy, table, weights, invalid, invalid_wsum, invalid_any, rgb_samps=None):
    """the tensor checks photometric_loss, photometric_loss_median and pixel_loss share: rgb (B, nv*3), rgb_gt (B, 3), the invalid-ray
    inputs, depth (B) with the smoothness term, thresh (B) when given -> _invalid_inputs' (policy, K, nv, masks)"""
    B = rgb_gt.shape[0]
    nv = rgb.shape[-1] // 3
    _req(rgb, "rgb", (B, nv * 3)), _req(rgb_gt, "rgb_gt", (B, 3))
    resolved = _invalid_inputs(invalid_policy, table, B, weights, invalid, invalid_wsum, invalid_any, rgb_samps, nv)
    if eas:
        _req(depth, "depth", (B,))
    if thresh is not None:
        _req(thresh, "thresh", (B,))
    return resolved


def _loss_args(rgb, depth, rgb_gt, parts, patch_h, patch_w, eas, scale_rgb, scale_eas, need_grad, with_depth, policy, K, nv, masks):
    """The BtsLossArgs of the l1+ssim entry points and the gradients it points to -> (args, g_rgb | None, g_depth | None); the last four
    arguments are _rgb_loss_inputs' result.  ``with_depth``: depth is handed over and gets its gradient -- photometric_loss says so whenever
    depth is given, photometric_loss_median only with the smoothness term."""
    depth = depth if with_depth else None
    g_rgb = torch.empty_like(rgb) if need_grad else None
    g_depth = torch.empty((rgb.shape[0],), device=rgb.device, dtype=torch.float32) if (need_grad and depth is not None) else None
    a = _lib.BtsLossArgs(rgb=rgb.data_ptr(), depth=_addr(depth), weights=_addr(masks["weights"]), invalid=_addr(masks["invalid"]),
                         rgb_gt=rgb_gt.data_ptr(), parts=parts.data_ptr(), g_rgb=_addr(g_rgb), g_depth=_addr(g_depth), n_patches=parts.shape[0],
                         patch_h=patch_h, patch_w=patch_w, nv=nv, K=K, invalid_policy=policy, edge_aware_smoothness=int(bool(eas)),
                         scale_rgb=scale_rgb, scale_eas=scale_eas, invalid_wsum=_addr(masks["invalid_wsum"]),
                         invalid_any=_addr(masks["invalid_any"]))
    return a, g_rgb, g_depth


def photometric_loss(rgb, depth, weights, invalid, rgb_gt, patch_h: int, patch_w: int, invalid_policy, eas: bool,
                     scale_rgb: float, scale_eas: float, need_grad: bool = True, invalid_wsum=None, invalid_any=None, thresh=None):
    """Patch-ordered renderer outputs -> per-patch partial sums and the loss gradients (bts_photometric_loss for patches of up to 64
    pixels, bts_photometric_loss_tiled above that: any (patch_h, patch_w), whole frames included).
    rgb (B, nv*3), depth (B) | None, weights (B, K) | None, invalid (B, K, nv) | None, rgb_gt (B, 3), thresh (B) | None: the
    automasking bound on every pixel's error (the _automask entry points)
    -> parts (B / (ph*pw), 4), g_rgb (B, nv*3) | None, g_depth (B) | None."""
    B = rgb_gt.shape[0]
    area = patch_h * patch_w
    if B % area:
        raise BtsNativeError(f"{B} rays are not a whole number of {patch_h}x{patch_w} patches")
    resolved = _rgb_loss_inputs(rgb, depth, rgb_gt, thresh, eas, invalid_policy, INVALID_POLICIES, weights, invalid, invalid_wsum, invalid_any)
    parts = torch.empty((B // area, 4), device=rgb.device, dtype=torch.float32)
    a, g_rgb, g_depth = _loss_args(rgb, depth, rgb_gt, parts, patch_h, patch_w, eas, scale_rgb, scale_eas, need_grad, True, *resolved)
    if area > WAVE_PATCH_PIXELS:
        # larger patches and whole frames: 16 x 16 tiles of each patch (bts_photometric_loss_tiled)
        return photometric_loss_tiled(a, parts, g_rgb, g_depth, _stream(rgb), thresh)
    if thresh is not None:
        _lib.check(_lib.load().bts_photometric_loss_automask(C.byref(a), _ptr(thresh), _stream(rgb)), "bts_photometric_loss_automask")
        return parts, g_rgb, g_depth
    _lib.check(_lib.load().bts_photometric_loss(C.byref(a), _stream(rgb)), "bts_photometric_loss")
    return parts, g_rgb, g_depth


def photometric_loss_tiled(a, parts, g_rgb, g_depth, stream, thresh=None):
    """bts_photometric_loss_tiled on a filled BtsLossArgs: any patch size, with a scratch workspace from torch's allocator (the library
    allocates nothing).  ``native.photometric_loss`` routes patches of more than 64 pixels here; tests call it directly to cross-check the
    two kernels on small patches."""
    lib = _lib.load()
    if thresh is not None:      # the same passes with the automasking bound (one more float per ray of workspace)
        ws = _scratch(parts.device, lib.bts_photometric_loss_tiled_automask_workspace(a.n_patches, a.patch_h, a.patch_w, a.nv))
        _lib.check(lib.bts_photometric_loss_tiled_automask(C.byref(a), _ptr(thresh), ws.data_ptr(), ws.numel(), stream),
                   "bts_photometric_loss_tiled_automask")
        return parts, g_rgb, g_depth
    ws = _scratch(parts.device, lib.bts_photometric_loss_tiled_workspace(a.n_patches, a.patch_h, a.patch_w, a.nv))
    _lib.check(lib.bts_photometric_loss_tiled(C.byref(a), ws.data_ptr(), ws.numel(), stream), "bts_photometric_loss_tiled")
    return parts, g_rgb, g_depth


def pixel_loss(rgb, depth, weights, invalid, rgb_gt, n: int, patch_h: int, patch_w: int, criterion: str, invalid_policy, median: bool,
               eas: bool, scale_rgb: float = 1.0, scale_eas: float = 1.0, need_grad: bool = True, invalid_wsum=None, invalid_any=None,
               rgb_samps=None, thresh=None):
    """The per-pixel criteria "l1" / "l2" of the reference's loss, with or without median thresholding, under any of its four invalid-ray
    policies, plus the edge-aware smoothness term (bts_pixel_loss, csrc/bts_loss_pixel.hip).  Flat layout of ``photometric_loss``:
    rgb (B, nv*3), depth (B) | None, weights (B, K) | None, invalid (B, K, nv) | None, rgb_samps (B, K, nv, 3) | None, rgb_gt (B, 3);
    ``n`` batch samples of B / n rays each, every sample a whole number of patch_h x patch_w patches.  thresh (B) | None: the automasking
    bound, one per ray, applied to each of its three channels before the keep factor and the median ranking (bts_pixel_loss_automask).
    -> out (4) = [rgb term, sum of the smoothness term, invalid rays, count], thresholds (n) | None, kept (1) int64 | None,
    g_rgb (B, nv*3) | None = scale_rgb * d out[0] / d rgb, g_depth (B) | None = scale_eas * d out[1] / d depth."""
    if criterion not in PIXEL_CRITERIA:
        raise BtsNativeError(f"pixel_loss: criterion {criterion!r} is not one of {sorted(PIXEL_CRITERIA)}")
    if invalid_policy not in PIXEL_POLICIES:
        raise BtsNativeError(f"pixel_loss: unknown invalid_policy {invalid_policy!r}")
    B = rgb_gt.shape[0]
    if n <= 0 or patch_h <= 0 or patch_w <= 0 or B % (n * patch_h * patch_w):
        raise BtsNativeError(f"{B} rays are not {n} samples of whole {patch_h}x{patch_w} patches")
    policy, K, nv, masks = _rgb_loss_inputs(rgb, depth, rgb_gt, thresh, eas, invalid_policy, PIXEL_POLICIES, weights, invalid, invalid_wsum,
                                            invalid_any, rgb_samps)
    dev = rgb.device
    out = torch.empty((4,), device=dev, dtype=torch.float32)
    thresholds = torch.empty((n,), device=dev, dtype=torch.float32) if median else None
    kept = torch.empty((1,), device=dev, dtype=torch.int64) if median else None
    g_rgb = torch.empty_like(rgb) if need_grad else None
    g_depth = torch.empty((B,), device=dev, dtype=torch.float32) if (need_grad and eas) else None
    a = _lib.BtsPixelLossArgs(rgb=rgb.data_ptr(), rgb_gt=rgb_gt.data_ptr(), depth=_addr(depth if eas else None),
                              **{name: _addr(t) for name, t in masks.items()}, out=out.data_ptr(),
                              thresholds=_addr(thresholds), kept=_addr(kept), g_rgb=_addr(g_rgb), g_depth=_addr(g_depth), B=B, n=n,
                              patch_h=patch_h, patch_w=patch_w, nv=nv, K=K, criterion=PIXEL_CRITERIA[criterion], invalid_policy=policy,
                              median_thresholding=int(bool(median)), edge_aware_smoothness=int(bool(eas)), scale_rgb=scale_rgb,
                              scale_eas=scale_eas)
    lib = _lib.load()
    ws = _scratch(dev, lib.bts_pixel_loss_workspace(B, n, patch_h, patch_w))
    if thresh is not None:
        _lib.check(lib.bts_pixel_loss_automask(C.byref(a), _ptr(thresh), ws.data_ptr(), ws.numel(), _stream(rgb)), "bts_pixel_loss_automask")
    else:
        _lib.check(lib.bts_pixel_loss(C.byref(a), ws.data_ptr(), ws.numel(), _stream(rgb)), "bts_pixel_loss")
    return out, thresholds, kept, g_rgb, g_depth


PIXEL_LOSS_MAX_CHANNELS = 27


def pixel_loss_channels(rgb, rgb_gt, weights, invalid, criterion: str, invalid_policy, scale_rgb: float = 1.0, need_grad: bool = True,
                        invalid_wsum=None, invalid_any=None):
    """Criterion "l1" / "l2" for C colour channels, 1 <= C <= 27 (bts_pixel_loss_channels, csrc/bts_loss_pixel_c.hip): rgb (B, nv*C),
    rgb_gt (B, C), weights (B, K) | None, invalid (B, K, nv) | None (or the renderer's per-ray reductions), invalid_policy none / strict /
    weight_guided -> out (4) = [rgb term = sum e / (B C), 0, invalid rays, B C], g_rgb (B, nv*C) | None = scale_rgb * d out[0] / d rgb."""
    if criterion not in PIXEL_CRITERIA:
        raise BtsNativeError(f"pixel_loss_channels: criterion {criterion!r} is not one of {sorted(PIXEL_CRITERIA)}")
    if invalid_policy not in PIXEL_POLICIES or PIXEL_POLICIES[invalid_policy] == 3:
        raise BtsNativeError(f"pixel_loss_channels: invalid_policy {invalid_policy!r} is not one of none / strict / weight_guided")
    _req(rgb_gt, "rgb_gt")
    B, ch = rgb_gt.shape
    if not 1 <= ch <= PIXEL_LOSS_MAX_CHANNELS or rgb.shape[-1] % ch:
        raise BtsNativeError(f"pixel_loss_channels: rgb_gt has {ch} channels (1 .. {PIXEL_LOSS_MAX_CHANNELS}), rgb {rgb.shape[-1]} per ray")
    nv = rgb.shape[-1] // ch
    _req(rgb, "rgb", (B, nv * ch))
    policy, K, nv, masks = _invalid_inputs(invalid_policy, PIXEL_POLICIES, B, weights, invalid, invalid_wsum, invalid_any, None, nv)
    dev = rgb.device
    out = torch.empty((4,), device=dev, dtype=torch.float32)
    g_rgb = torch.empty_like(rgb) if need_grad else None
    a = _lib.BtsPixelLossArgs(rgb=rgb.data_ptr(), rgb_gt=rgb_gt.data_ptr(), **{name: _addr(t) for name, t in masks.items()}, out=out.data_ptr(),
                              g_rgb=_addr(g_rgb), B=B, n=1, patch_h=1, patch_w=1, nv=nv, K=K, criterion=PIXEL_CRITERIA[criterion],
                              invalid_policy=policy, scale_rgb=scale_rgb, scale_eas=0.0)
    lib = _lib.load()
    ws = _scratch(dev, lib.bts_pixel_loss_channels_workspace(B))
    _lib.check(lib.bts_pixel_loss_channels(C.byref(a), ch, ws.data_ptr(), ws.numel(), _stream(rgb)), "bts_pixel_loss_channels")
    return out, g_rgb


def photometric_loss_median(rgb, depth, weights, invalid, rgb_gt, n: int, patch_h: int, patch_w: int, invalid_policy, eas: bool,
                            scale_rgb: float = 1.0, scale_eas: float = 1.0, need_grad: bool = True, invalid_wsum=None, invalid_any=None,
                            thresh=None, parts=None):
    """Criterion "l1+ssim" with median thresholding (bts_photometric_loss_median, csrc/bts_loss_tiled.hip): the flat layout of
    ``photometric_loss`` -- rgb (B, nv*3), depth (B) | None, weights (B, K) | None, invalid (B, K, nv) | None, rgb_gt (B, 3), thresh (B) |
    None (the automasking bound) -- in ``n`` batch samples of B / n rays each, every sample a whole number of patch_h x patch_w patches of
    any size.  ``parts`` (B / (ph*pw), 4) | None: receives the per-patch sums [e before thresholding, smoothness term, invalid rays, 0]
    (allocated here when not given).
    -> out (4) = [sum of kept e / count, sum of the smoothness term, invalid rays, count], thresholds (n), kept (1) int64,
    g_rgb (B, nv*3) | None = scale_rgb * d out[0] / d rgb, g_depth (B) | None = scale_eas * d out[1] / d depth."""
    if invalid_policy not in INVALID_POLICIES:
        raise BtsNativeError(f"photometric_loss_median: invalid_policy {invalid_policy!r} is not one of none / strict / weight_guided (the "
                             "diverse rule goes in as invalid_any under strict: loss_diverse_flags)")
    B = rgb_gt.shape[0]
    area = patch_h * patch_w
    if n <= 0 or area <= 0 or B % (n * area):
        raise BtsNativeError(f"{B} rays are not {n} samples of whole {patch_h}x{patch_w} patches")
    resolved = _rgb_loss_inputs(rgb, depth, rgb_gt, thresh, eas, invalid_policy, INVALID_POLICIES, weights, invalid, invalid_wsum, invalid_any)
    dev = rgb.device
    if parts is None:
        parts = torch.empty((B // area, 4), device=dev, dtype=torch.float32)
    _req(parts, "parts", (B // area, 4))
    out = torch.empty((4,), device=dev, dtype=torch.float32)
    thresholds = torch.empty((n,), device=dev, dtype=torch.float32)
    kept = torch.empty((1,), device=dev, dtype=torch.int64)
    a, g_rgb, g_depth = _loss_args(rgb, depth, rgb_gt, parts, patch_h, patch_w, eas, scale_rgb, scale_eas, need_grad, bool(eas), *resolved)
    lib = _lib.load()
    ws = _scratch(dev, lib.bts_photometric_loss_median_workspace(B // area, patch_h, patch_w, a.nv, n))
    _lib.check(lib.bts_photometric_loss_median(C.byref(a), n, _ptr(thresh), _ptr(out), _ptr(thresholds), _ptr(kept), ws.data_ptr(), ws.numel(),
                                               _stream(rgb)), "bts_photometric_loss_median")
    return out, thresholds, kept, g_rgb, g_depth


def loss_regularisers(alphas, depth, **kw):
    """-> (terms, reg, g_alphas | None, g_depth | None) of ``loss_regularisers_packed``"""
    return loss_regularisers_packed(alphas, depth, **kw)[:4]


def loss_regularisers_packed(alphas, depth, *, n: int, pc: int, ph: int, pw: int, policy, weights=None, invalid=None, invalid_wsum=None,
                             invalid_any=None, rgb_samps=None, coef, alpha_reg_reduction: str = "ray", alpha_reg_fraction: float = 1 / 8,
                             need_grad: bool = True):
    """The optional regularisers of the reference's loss for one scale (bts_loss_regularisers, csrc/bts_loss_reg.hip): alphas (B, K),
    depth (B) | None in the flat patch layout of ``photometric_loss`` (B = n * pc * ph * pw); the invalid-ray inputs of scale 0 in one of
    the forms ``pixel_loss`` takes -- weights (B, Ki) / invalid (B, Ki, nv), invalid_wsum / invalid_any (B, nv), or with
    weight_guided_diverse rgb_samps (B, Ki, nv, 3) too.  coef = (alpha_reg, surfaceness, entropy, depth): a term runs when its coefficient
    is > 0 (the caller passes lambda / n_scales, the entropy's undivided and at scale 0 only).
    alphas may be None when no alpha term is on (a lean render dict with the depth term alone).
    -> terms (5) = [alpha_reg, surfaceness, entropy, depth term, invalid rays], reg (1) = sum_t coef_t terms_t,
    g_alphas (B, K) | None = d reg / d alphas (with an alpha term), g_depth (B) | None = d reg / d depth (with the depth term), and the
    (6,) tensor terms and reg are views of.  Asynchronous on the current stream."""
    if policy not in PIXEL_POLICIES:
        raise BtsNativeError(f"loss_regularisers: unknown invalid_policy {policy!r}")
    if alpha_reg_reduction not in ("ray", "slice"):
        raise BtsNativeError(f"loss_regularisers: alpha_reg_reduction {alpha_reg_reduction!r} is not 'ray' or 'slice'")
    c_alpha, c_surf, c_ent, c_depth = (float(c) for c in coef)
    alpha_on, depth_on = c_alpha > 0 or c_surf > 0 or c_ent > 0, c_depth > 0
    if depth_on and (ph < 2 or pw < 2):
        raise ValueError(f"loss_regularisers: the depth term (lambda_depth_reg / lambda_depth_smoothness) needs patches of at least 2 x 2 "
                         f"pixels, got {ph} x {pw}: the reference's mean over an empty set of differences is NaN (BTS_E_UNSUPPORTED)")
    if alpha_on or alphas is not None:
        _req(alphas, "alphas")
        if alphas.dim() != 2:
            raise BtsNativeError(f"alphas: expected (B, K), got {tuple(alphas.shape)}")
        B, K = alphas.shape
    else:
        _req(depth, "depth")
        B, K = depth.shape[0], 2
    if n <= 0 or pc <= 0 or ph <= 0 or pw <= 0 or B != n * pc * ph * pw:
        raise BtsNativeError(f"{B} rays are not {n} x {pc} patches of {ph}x{pw}")
    pol, Ki, nv, masks = _invalid_inputs(policy, PIXEL_POLICIES, B, weights, invalid, invalid_wsum, invalid_any, rgb_samps)
    if depth_on:
        _req(depth, "depth", (B,))
    dev = (alphas if alphas is not None else depth).device
    out = torch.empty((6,), device=dev, dtype=torch.float32)
    g_alphas = torch.empty_like(alphas) if (need_grad and alpha_on) else None
    g_depth = torch.empty((B,), device=dev, dtype=torch.float32) if (need_grad and depth_on) else None
    a = _lib.BtsLossRegArgs(alphas=_addr(alphas), depth=_addr(depth if depth_on else None), **{name: _addr(t) for name, t in masks.items()},
                            terms=out.data_ptr(), reg=out.data_ptr() + 20, g_alphas=_addr(g_alphas), g_depth=_addr(g_depth), B=B,
                            n_patches=n * pc, patch_h=ph, patch_w=pw, nv=nv, K=K, K_invalid=Ki, invalid_policy=pol,
                            alpha_reg_slice=int(alpha_reg_reduction == "slice"), alpha_reg_fraction=alpha_reg_fraction,
                            coef_alpha_reg=c_alpha, coef_surfaceness=c_surf, coef_entropy=c_ent, coef_depth=c_depth)
    lib = _lib.load()
    ws = _scratch(dev, lib.bts_loss_regularisers_workspace(B, n * pc, ph, pw, K))
    _lib.check(lib.bts_loss_regularisers(C.byref(a), ws.data_ptr(), ws.numel(), _stream(out)), "bts_loss_regularisers")
    return out[:5], out[5:], g_alphas, g_depth, out


def automask_errors(images: torch.Tensor, ids_loss, scale: float = 0.5, want_errors: bool = True, want_images4: bool = False):
    """The error map of use_automasking (trainer.py:203-206; bts_automask_errors, csrc/bts_automask.hip): images (n, v, 3, H, W), the
    processed frames in [0, 1]; ids_loss: 1 .. BTS_MAX_VIEWS frame indices in [0, v) -> errors (n, v, H, W) | None, images4
    (n, v, 4, H, W) | None (the frames with the map as their fourth plane), one launch."""
    _req(images, "images")
    if images.dim() != 5 or images.shape[2] != 3:
        raise BtsNativeError(f"images: expected (n, v, 3, H, W), got {tuple(images.shape)}")
    n, v, _, H, W = images.shape
    ids = [int(i) for i in ids_loss]
    arr = (C.c_int32 * max(len(ids), 1))(*ids)
    errors = torch.empty((n, v, H, W), device=images.device, dtype=torch.float32) if want_errors else None
    images4 = torch.empty((n, v, 4, H, W), device=images.device, dtype=torch.float32) if want_images4 else None
    _lib.check(_lib.load().bts_automask_errors(_ptr(images), n, v, H, W, arr, len(ids), scale, _ptr(errors), _ptr(images4), _stream(images)),
               "bts_automask_errors")
    return errors, images4


def loss_diverse_flags(rgb_samps, weights, invalid):
    """The per-(ray, view) flag of invalid_policy weight_guided_diverse as 0 / 1 floats (bts_loss_diverse_flags):
    rgb_samps (B, K, nv, 3), weights (B, K), invalid (B, K, nv) -> (B, nv)."""
    B, K, nv = invalid.shape
    _req(invalid, "invalid", (B, K, nv)), _req(weights, "weights", (B, K)), _req(rgb_samps, "rgb_samps", (B, K, nv, 3))
    flags = torch.empty((B, nv), device=invalid.device, dtype=torch.float32)
    _lib.check(_lib.load().bts_loss_diverse_flags(_ptr(rgb_samps), _ptr(weights), _ptr(invalid), B, K, nv, _ptr(flags), _stream(invalid)),
               "bts_loss_diverse_flags")
    return flags


def sample_coarse(rays: torch.Tensor, u: torch.Tensor, lindisp: bool) -> torch.Tensor:
    """rays (B,8), u (B,K) uniform jitter -> z_samp (B,K) (bts_sample_coarse)."""
    B, K = u.shape
    _req(rays, "rays", (B, 8)), _req(u, "u")
    out = torch.empty_like(u)
    _lib.check(_lib.load().bts_sample_coarse(_ptr(rays), _ptr(u), B, K, int(lindisp), _ptr(out), _stream(out)),
               "bts_sample_coarse")
    return out


def sample_fine(rays, weights, z_coarse, depth, u, t, noise, depth_std: float, lindisp: bool, nan_count=None):
    """NeRFRenderer.sample_fine / sample_fine_depth and their merge with the coarse depths in one launch (bts_sample_fine,
    csrc/bts_sample_fine.hip).  rays (B, 8); weights (B, Kc), u, t (B, n_imp) or all None (no importance draws); depth (B), noise
    (B, Kfd) or both None (no depth draws); nan_count: an int32 tensor of one element the NaNs among the produced samples are added to,
    or None.  With z_coarse (B, Kc) -> the sorted union (B, Kc + n_imp + Kfd); with z_coarse None -> (importance | None, depth | None),
    unsorted.  Asynchronous on the current stream."""
    _req(rays, "rays")
    B = rays.shape[0]
    _req(rays, "rays", (B, 8))
    n_imp = 0 if u is None else u.shape[-1]
    Kfd = 0 if noise is None else noise.shape[-1]
    if n_imp + Kfd == 0:
        raise BtsNativeError("sample_fine: neither importance draws (u, t) nor depth draws (noise) were given")
    for name, x in (("weights", weights if n_imp else None), ("z_coarse", z_coarse)):
        if x is not None:
            _req(x, name)
    # the per-ray count of the weights / coarse depths (the depth draws alone have none of their own: the smallest the entry takes)
    Kc = weights.shape[-1] if n_imp else (z_coarse.shape[-1] if z_coarse is not None else 2)
    if n_imp:
        _req(weights, "weights", (B, Kc)), _req(u, "u", (B, n_imp)), _req(t, "t", (B, n_imp))
    if z_coarse is not None:
        _req(z_coarse, "z_coarse", (B, Kc))
    if Kfd:
        _req(depth, "depth", (B,)), _req(noise, "noise", (B, Kfd))
    if nan_count is not None:
        _req_as(nan_count, "nan_count", torch.int32, (1,))
    dev = rays.device
    if z_coarse is not None:
        out, out_d = torch.empty((B, Kc + n_imp + Kfd), device=dev, dtype=torch.float32), None
    else:
        out = torch.empty((B, n_imp), device=dev, dtype=torch.float32) if n_imp else None
        out_d = torch.empty((B, Kfd), device=dev, dtype=torch.float32) if Kfd else None
    a = _lib.BtsSampleFineArgs(rays=_addr(rays), weights=_addr(weights if n_imp else None), z_coarse=_addr(z_coarse), depth=_addr(depth if Kfd else None),
                               u=_addr(u), t=_addr(t), noise=_addr(noise), z_out=_addr(out), z_depth_out=_addr(out_d), nan_count=_addr(nan_count),
                               B=B, mode=_lib.BTS_SAMPLE_FINE, Kc=Kc, n_coarse=Kc, Kf=n_imp + Kfd, Kfd=Kfd, lindisp=int(bool(lindisp)), sorted=1,
                               depth_std=float(depth_std))
    _lib.check(_lib.load().bts_sample_fine(C.byref(a), _stream(rays)), "bts_sample_fine")
    return out if z_coarse is not None else (out, out_d)


def sample_coarse_from_dist(weights, z_samp, u, t, lindisp: bool, sort: bool = False, nan_count=None):
    """NeRFRenderer.sample_coarse_from_dist (bts_sample_fine in from-dist mode): weights, z_samp (B, ns), u, t (B, n_coarse) in [0, 1)
    -> (B, n_coarse), ascending with ``sort``.  n_coarse > ns is an error (the reference raises there)."""
    _req(weights, "weights"), _req(u, "u")
    if weights.dim() != 2 or u.dim() != 2:
        raise BtsNativeError(f"sample_coarse_from_dist: expected weights (B, ns) and u (B, n_coarse), got {tuple(weights.shape)}, {tuple(u.shape)}")
    (B, ns), n_coarse = weights.shape, u.shape[1]
    _req(z_samp, "z_samp", (B, ns)), _req(u, "u", (B, n_coarse)), _req(t, "t", (B, n_coarse))
    if nan_count is not None:
        _req_as(nan_count, "nan_count", torch.int32, (1,))
    out = torch.empty((B, n_coarse), device=weights.device, dtype=torch.float32)
    a = _lib.BtsSampleFineArgs(weights=_addr(weights), z_coarse=_addr(z_samp), u=_addr(u), t=_addr(t), z_out=_addr(out), nan_count=_addr(nan_count), B=B,
                               mode=_lib.BTS_SAMPLE_FROM_DIST, Kc=ns, n_coarse=n_coarse, lindisp=int(bool(lindisp)), sorted=int(bool(sort)))
    _lib.check(_lib.load().bts_sample_fine(C.byref(a), _stream(out)), "bts_sample_fine")
    return out


def invert_small(m: torch.Tensor) -> torch.Tensor:
    """(..., d, d) with d in {3, 4} -> inverses (bts_invert_small); the stand-in for torch.inverse on poses / intrinsics."""
    d = m.shape[-1]
    if m.shape[-2] != d or d not in (3, 4):
        raise BtsNativeError(f"invert_small: expected (..., 3, 3) or (..., 4, 4), got {tuple(m.shape)}")
    src = m.float().contiguous()
    _req(src, "matrices")
    out = torch.empty_like(src)
    N = src.numel() // (d * d)
    _lib.check(_lib.load().bts_invert_small(_ptr(src), _ptr(out), N, d, _stream(src)), "bts_invert_small")
    return out


def distance_to_z(depths: torch.Tensor, projs: torch.Tensor) -> torch.Tensor:
    """depths (n,nv,H,W), projs (n,nv,3,3) -> z (n,nv,H,W) (bts_invert_small + bts_distance_to_z)."""
    n, nv, H, W = depths.shape
    _req(depths, "depths")
    inv_K = invert_small(projs).reshape(n * nv, 3, 3)
    _req(inv_K, "inv_K", (n * nv, 3, 3))
    out = torch.empty_like(depths)
    _lib.check(_lib.load().bts_distance_to_z(_ptr(depths), _ptr(inv_K), n * nv, H, W, _ptr(out), _stream(out)),
               "bts_distance_to_z")
    return out


# --------------------------------------------------------------------------------------------------------------
# field state handed to the renderer
# --------------------------------------------------------------------------------------------------------------
def _spec_cfg(spec: FieldSpec, n=1, H=1, W=1, nv=0, feat_shift=0, enc_view=-1) -> BtsFieldCfg:
    return BtsFieldCfg(n=n, H=H, W=W, C=spec.C, d_hidden=spec.d_hidden, n_blocks=spec.n_blocks, nv=nv, num_freqs=spec.num_freqs,
                       code_mode={"z": 0, "distance": 1}[spec.code_mode], inv_z=int(spec.inv_z), learn_empty=int(spec.learn_empty),
                       empty_empty=int(spec.empty_empty), freq_factor=spec.freq_factor, d_min=spec.d_min, d_max=spec.d_max,
                       feat_shift=feat_shift, enc_render_view=enc_view if 0 <= enc_view < nv else -1, tile_blocks=int(spec.tile_blocks))


def proj_storage_order(d_hidden: int) -> torch.Tensor:
    """order[s] = hidden unit stored at channel s of proj_nhwc (bts_common.h: proj_hidden_of_storage): within each group of 32
    hidden units the renderer keeps the 16 accumulator rows of one lane half contiguous."""
    s = torch.arange(d_hidden)
    ht, r = s // 32, s % 32
    h, q, e = r // 16, (r // 4) % 4, r % 4
    return ht * 32 + 8 * q + 4 * h + e


def is_channels_last(t: torch.Tensor) -> bool:
    """A 4-d tensor whose memory is (N, H, W, C) -- torch's channels_last format -- and not also plain contiguous (C = 1 or H = W = 1)."""
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def as_feature_map(t: torch.Tensor) -> torch.Tensor:
    """The encoder's map as the library takes it: fp32, dense, in the layout it ALREADY has when that is NCHW or channels-last (ABI 8:
    bts_project_features_cl -- the format MIOpen's NHWC convolutions and bts_conv3x3_fwd write), a contiguous copy otherwise."""
    t = t.float()
    return t if (t.is_contiguous() or is_channels_last(t)) else t.contiguous()


def project_features(spec: FieldSpec, feat_nchw: torch.Tensor, mlp_params: torch.Tensor, tiles: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F (N,C,H,W) -> G (N,H,W,Hd) = F . w_in[:, :C]^T with the channels in storage order (proj_storage_order)
    (bts_project_features).  With ``tiles`` (N, proj_tile_count) uint8 only the flagged 64-texel tiles are evaluated and the rest of G
    is UNINITIALISED (bts_project_features_tiles): a map for the render whose samples ``mark_sampled_tiles`` flagged, nothing else.
    A channels_last F (memory (N,H,W,C)) is read as it is (bts_project_features_cl): the same G to fp32 rounding (another summation order)."""
    N, Cc, H, W = feat_nchw.shape
    cl = is_channels_last(feat_nchw)
    if cl:
        _req(feat_nchw.permute(0, 2, 3, 1), "feat (channels_last)", (N, H, W, spec.C))
    else:
        _req(feat_nchw, "feat_nchw", (N, spec.C, H, W))
    _req(mlp_params, "mlp_params", (spec.mlp_param_count(),))
    out = torch.empty((N, H, W, spec.d_hidden), device=feat_nchw.device, dtype=torch.float32)
    cfg = _spec_cfg(spec, N, H, W)
    if tiles is not None:
        _req_tiles(tiles, N * proj_tile_count(spec, H, W), out.device, "the map's")
    if cl:
        _lib.check(_lib.load().bts_project_features_cl(C.byref(cfg), _ptr(feat_nchw), _ptr(mlp_params), N, _ptr(tiles), _ptr(out), _stream(out)),
                   "bts_project_features_cl")
    elif tiles is not None:
        _lib.check(_lib.load().bts_project_features_tiles(C.byref(cfg), _ptr(feat_nchw), _ptr(mlp_params), N, _ptr(tiles), _ptr(out), _stream(out)),
                   "bts_project_features_tiles")
    else:
        _lib.check(_lib.load().bts_project_features(C.byref(cfg), _ptr(feat_nchw), _ptr(mlp_params), N, _ptr(out), _stream(out)),
                   "bts_project_features")
    return out


def mark_sampled_tiles(spec: FieldSpec, n: int, H: int, W: int, feat_shift: int, K_enc, w2c_enc, rays, z_samp=None, jitter=None, lindisp=True):
    """Flags (n, tiles per image of the (H >> s, W >> s) map) uint8 of the 64-texel tiles of the projected map that a render of
    ``rays`` (n*Bp, 8) at the depths ``z_samp`` (n*Bp, K) -- or, as bts_render_fwd forms them, from ``jitter`` -- reads
    (bts_mark_sampled_tiles: the render kernels' own routines, the same texels bit for bit)."""
    src = z_samp if z_samp is not None else jitter
    _req(rays, "rays", (src.shape[0], 8)), _req(src, "z_samp / jitter"), _req(K_enc, "K_enc", (n, 3, 3)), _req(w2c_enc, "w2c_enc", (n, 4, 4))
    cfg = _spec_cfg(spec, n, H, W, feat_shift=feat_shift)
    tiles = torch.zeros((n, proj_tile_count(spec, H >> feat_shift, W >> feat_shift)), device=rays.device, dtype=torch.uint8)
    args = BtsRenderArgs(rays_per_sample=rays.shape[0] // n, K=src.shape[1], rays=rays.data_ptr(), z_samp=_addr(z_samp),
                         jitter=_addr(jitter if z_samp is None else None), lindisp=int(bool(lindisp)), reserved_=0)
    _lib.check(_lib.load().bts_mark_sampled_tiles(C.byref(cfg), _ptr(K_enc), _ptr(w2c_enc), C.byref(args), _ptr(tiles), _stream(rays)),
               "bts_mark_sampled_tiles")
    return tiles


def project_features_bwd(spec: FieldSpec, feat_nchw, d_proj, mlp_params, need_feat=True, need_mlp=True, tiles=None, clear_after=False):
    """-> (d_feat_nchw | None, d_mlp_params | None) (bts_project_features_bwd).  With ``tiles`` (N, proj_tile_count) uint8 -- the flags
    ``render_bwd`` set next to a d_proj that was all zero before -- only the flagged 64-texel tiles of d_proj are read
    (bts_project_features_bwd_tiles); ``clear_after`` returns the pair to all zero.  For a channels_last F the gradient comes back
    channels_last as well (bts_project_features_bwd_cl): same values, a 64-texel tile of either is one contiguous piece."""
    N, Cc, H, W = feat_nchw.shape
    cl = is_channels_last(feat_nchw)
    if cl:
        _req(feat_nchw.permute(0, 2, 3, 1), "feat (channels_last)")
    else:
        _req(feat_nchw, "feat_nchw")
    _req(d_proj, "d_proj", (N, H, W, spec.d_hidden)), _req(mlp_params, "mlp_params")
    d_feat = torch.empty_like(feat_nchw) if need_feat else None          # (preserve_format: channels_last stays channels_last)
    d_mlp = torch.zeros_like(mlp_params) if need_mlp else None
    cfg = _spec_cfg(spec, N, H, W)
    lib = _lib.load()
    if tiles is not None:
        _req_tiles(tiles, N * proj_tile_count(spec, H, W), d_proj.device, "d_proj's")
    if cl:
        _lib.check(lib.bts_project_features_bwd_cl(C.byref(cfg), _ptr(feat_nchw), _ptr(d_proj), _ptr(tiles), _ptr(mlp_params), N, _ptr(d_feat),
                                                   _ptr(d_mlp), 1 if (clear_after and tiles is not None) else 0, _stream(d_proj)),
                   "bts_project_features_bwd_cl")
    elif tiles is not None:
        _lib.check(lib.bts_project_features_bwd_tiles(C.byref(cfg), _ptr(feat_nchw), _ptr(d_proj), _ptr(tiles), _ptr(mlp_params), N, _ptr(d_feat),
                                                      _ptr(d_mlp), 1 if clear_after else 0, _stream(d_proj)), "bts_project_features_bwd_tiles")
    else:
        _lib.check(lib.bts_project_features_bwd(C.byref(cfg), _ptr(feat_nchw), _ptr(d_proj), _ptr(mlp_params), N, _ptr(d_feat),
                                                _ptr(d_mlp), _stream(d_proj)), "bts_project_features_bwd")
    return d_feat, d_mlp


def proj_tile_map(H: int, W: int, blocks: bool = False) -> torch.Tensor:
    """(H, W) int64: the tile (0 .. proj_tile_count - 1) of every texel of an (H, W) projected map -- the geometry of csrc/bts_common.h:
    ``blocks`` (FieldSpec.tile_blocks) and H a multiple of 4, W of 16: blocks of 4 rows x 16 texels, numbered row-major; else 64
    consecutive texels of the row-major map.  What `tiles` flags mean; ``flags[:, proj_tile_map(H, W, blocks)]`` is the per-texel mask."""
    if blocks and H % 4 == 0 and W % 16 == 0:
        y, x = torch.arange(H).view(-1, 1), torch.arange(W).view(1, -1)
        return (y // 4) * (W // 16) + (x // 16)
    return (torch.arange(H * W) // 64).view(H, W)


def proj_tile_count(spec: FieldSpec, H: int, W: int) -> int:
    """Tiles (64 texels each: proj_tile_map) per image of an (H, W) projected map (bts_proj_tile_count)."""
    cfg = _spec_cfg(spec, 1, H, W)
    n = int(_lib.load().bts_proj_tile_count(C.byref(cfg)))
    if n < 0:
        raise BtsNativeError(f"bts_proj_tile_count: {_lib.load().bts_last_error().decode(errors='replace')}")
    return n


class FieldTensors:
    """Device tensors in the layouts of include/bts_render.h.  ``proj_nhwc`` (G) may require grad: it is produced by
    ``ProjectFunction`` from the encoder output and the MLP parameters inside autograd.
    ``feat_shift`` = s: the map is the decoder's scale-s output at ITS size (n, H >> s, W >> s, .) and is read as its nearest-neighbour
    resize to H x W -- what models_bts.py:115-117 materialises -- without the resize (BtsFieldCfg.feat_shift)."""

    def __init__(self, spec: FieldSpec, proj_nhwc, K_enc, w2c_enc, imgs_nhwc4, K_r, w2c_r, empty_feature=None, feat_nhwc=None, feat_shift=0,
                 enc_view=-1):
        """enc_view: index of the render view whose camera is the encoder camera (BtsFieldCfg.enc_render_view), -1 = none / unknown."""
        ref = proj_nhwc if proj_nhwc is not None else feat_nhwc
        n, H, W, ch = ref.shape
        H, W = H << feat_shift, W << feat_shift
        if feat_shift and proj_nhwc is None:
            raise BtsNativeError("feat_shift > 0 needs the projected map")
        if proj_nhwc is not None and ch != spec.d_hidden:
            raise BtsNativeError(f"proj_nhwc has {ch} channels, spec says d_hidden={spec.d_hidden}")
        if proj_nhwc is None and ch != spec.C:
            raise BtsNativeError(f"feat_nhwc has {ch} channels, spec says C={spec.C}")
        nv = 0 if imgs_nhwc4 is None else imgs_nhwc4.shape[1]
        if spec.mlp_color:
            # the MLP predicts the one colour (nv = 1, models_bts.py:321): no frames, no render cameras
            if proj_nhwc is None:
                raise BtsNativeError("MLP-predicted colour needs the projected feature map")
            imgs_nhwc4 = K_r = w2c_r = None
            nv, enc_view = 1, -1
        _req(ref.detach(), "proj_nhwc/feat_nhwc"), _req(K_enc, "K_enc", (n, 3, 3)), _req(w2c_enc, "w2c_enc", (n, 4, 4))
        if nv and not spec.mlp_color:
            _req(imgs_nhwc4, "imgs_nhwc4", (n, nv, H, W, 4)), _req(K_r, "K_r", (n, nv, 3, 3)), _req(w2c_r, "w2c_r", (n, nv, 4, 4))
        if nv > _lib.BTS_MAX_VIEWS:
            raise BtsNativeError(f"nv={nv} render views exceed BTS_MAX_VIEWS={_lib.BTS_MAX_VIEWS}")
        if spec.learn_empty:
            if empty_feature is None:
                raise BtsNativeError("learn_empty needs empty_feature")
            _req(empty_feature.detach(), "empty_feature", (spec.C,))
        self.spec, self.n, self.H, self.W, self.nv, self.feat_shift = spec, n, H, W, nv, feat_shift
        self.enc_view = enc_view
        self.proj_nhwc, self.feat_nhwc, self.K_enc, self.w2c_enc = proj_nhwc, feat_nhwc, K_enc, w2c_enc
        self.imgs_nhwc4, self.K_r, self.w2c_r = imgs_nhwc4, K_r, w2c_r
        self.empty_feature = empty_feature
        self.proj_link = None   # ProjLink when proj_nhwc came out of ProjectFunction (field.py): see SPARSE_PROJ_GRAD
        # (rays data_ptr, z / jitter data_ptr, rows) of the ONE sample set a sparsely projected map is valid for (BTSNet.native_field(
        # sampled=...): only the tiles those samples read were projected, the rest of proj_nhwc is uninitialised memory), else None.
        # field_query / occupancy_profile reject a partial map, render_fwd / render_bwd check the sample set.
        self.partial = None
        # 3 when the frames stand for PatchProcessor(3)'s 27-channel output (BTSNet native_patch_color): the colours then come from the
        # bts_patch_color_* entries behind the render (PatchColorFunction); 0 = the frames' own three channels
        self.patch = 0

    @property
    def mlp_color(self) -> bool:
        """True for a four-output MLP that predicts the colour (sample_color=False): render_fwd / render_bwd / field_query then take the
        bts_*_mlp_color entries."""
        return self.spec.mlp_color

    def cfg(self, nv=None) -> BtsFieldCfg:
        return _spec_cfg(self.spec, self.n, self.H, self.W, self.nv if nv is None else nv, self.feat_shift, self.enc_view)

    def tensors(self, mlp_params: torch.Tensor) -> BtsFieldTensors:
        return BtsFieldTensors(feat_nhwc=_addr(self.feat_nhwc), proj_nhwc=_addr(self.proj_nhwc), K_enc=_addr(self.K_enc), w2c_enc=_addr(self.w2c_enc),
                               imgs_nhwc4=_addr(self.imgs_nhwc4), K_r=_addr(self.K_r), w2c_r=_addr(self.w2c_r),
                               empty_feature=_addr(self.empty_feature), mlp_params=mlp_params.data_ptr())


def group_tables(groups, n_views: int, singles_twice: bool):
    """View groups as BtsMultiViewField takes them: ``groups`` = lists of view positions (torch_modes._merge_groups' argument), or None
    for no merge (every view its own group, counted once: the plain mean) -> (start, member, mult).  ``singles_twice``: a one-member
    group of a merged field is counted twice (the reference's feature merge, models_bts.py:196-209)."""
    merged = groups is not None
    groups = [[int(v) for v in g] for g in groups] if merged else [[v] for v in range(n_views)]
    start, member, mult = [0], [], []
    for g in groups:
        member += g
        start.append(len(member))
        mult.append(2 if (merged and singles_twice and len(g) == 1) else 1)
    return start, member, mult


class MultiViewField:
    """Several encoder views merged per point (BtsMultiViewField): ``views`` = one ordinary ``FieldTensors`` per encoder view, all of
    one spec and size (view 0 carries the render views' frames and cameras); ``enc_groups`` / ``ren_groups`` = lists of view positions
    as ``torch_modes._merge_groups`` takes them, or None (no merge).  ``nv`` is nv', the number of render groups."""

    mlp_color = False
    partial = None
    proj_link = None

    def __init__(self, views, enc_groups=None, ren_groups=None):
        views = list(views)
        if not 1 <= len(views) <= _lib.BTS_MV_MAX_VIEWS:
            raise BtsNativeError(f"{len(views)} encoder views; 1 .. {_lib.BTS_MV_MAX_VIEWS} are supported")
        v0 = views[0]
        for i, v in enumerate(views):
            if v.proj_nhwc is None:
                raise BtsNativeError(f"encoder view {i}: merged encoder views need the projected feature map")
            if v.spec.mlp_color:
                raise BtsNativeError("merged encoder views with MLP-predicted colour are served by the PyTorch composition only")
        if v0.nv < 1:
            raise BtsNativeError("merged encoder views need at least one render view")
        self.views, self.spec, self.n, self.H, self.W, self.feat_shift = views, v0.spec, v0.n, v0.H, v0.W, v0.feat_shift
        self.enc_tables = group_tables(enc_groups, len(views), True)
        self.ren_tables = group_tables(ren_groups, v0.nv, False)
        self.nv = len(self.ren_tables[2])
        self.empty_feature = v0.empty_feature

    @property
    def proj_maps(self):
        return [v.proj_nhwc for v in self.views]

    @property
    def proj_nhwc(self):
        return self.views[0].proj_nhwc

    def struct(self, mlp_params: torch.Tensor) -> "_lib.BtsMultiViewField":
        mv = _lib.BtsMultiViewField()
        mv.V = len(self.views)
        for i, v in enumerate(self.views):
            mv.cfg[i], mv.view[i] = v.cfg(), v.tensors(mlp_params)
        (es, em, ek), (rs, rm, _) = self.enc_tables, self.ren_tables
        mv.n_enc_groups, mv.n_ren_groups = len(ek), len(rs) - 1
        for name, vals in (("enc_group_start", es), ("enc_member", em), ("enc_mult", ek), ("ren_group_start", rs), ("ren_member", rm)):
            if len(vals) > len(getattr(mv, name)):
                raise BtsNativeError(f"{name}: {len(vals)} entries exceed the table ({len(getattr(mv, name))})")
            for i, x in enumerate(vals):
                getattr(mv, name)[i] = x
        return mv


def check_supported(spec: FieldSpec, nv: int = 1):
    cfg = _spec_cfg(spec, nv=nv)
    if not _lib.load().bts_supported(C.byref(cfg)):
        raise BtsNativeError(f"field shape outside the compiled envelope: C={spec.C} d_hidden={spec.d_hidden} "
                             f"n_blocks={spec.n_blocks} num_freqs={spec.num_freqs} nv={nv}")


# --------------------------------------------------------------------------------------------------------------
# render forward / backward
# --------------------------------------------------------------------------------------------------------------
_OUT_KEYS = ("rgb", "depth", "weights", "alphas", "invalid", "rgb_samps", "sigma_raw", "trans", "invalid_wsum", "invalid_any")


def _render_args(ft: FieldTensors, rays, z_samp, hard_alpha_cap, white_bkgd, outs, sigma_noise=None, jitter=None, lindisp=True):
    K = (z_samp if z_samp is not None else jitter).shape[1]
    if sigma_noise is not None:
        _req(sigma_noise, "sigma_noise", (rays.shape[0], K))
    return BtsRenderArgs(rays_per_sample=rays.shape[0] // ft.n, K=K, hard_alpha_cap=int(hard_alpha_cap),
                         white_bkgd=int(white_bkgd), rays=rays.data_ptr(), z_samp=_addr(z_samp), sigma_noise=_addr(sigma_noise),
                         jitter=_addr(jitter), lindisp=int(bool(lindisp)), reserved_=0, z_samp_out=_addr(outs.get("z_samp")),
                         **{k: _addr(outs.get(k)) for k in _OUT_KEYS})


def render_fwd(ft: FieldTensors, mlp_params: torch.Tensor, rays: torch.Tensor, z_samp: torch.Tensor, *, hard_alpha_cap: bool,
               white_bkgd: bool = False, want_weights=False, want_alphas=False, want_invalid=True, want_rgb_samps=False,
               want_saved=False, want_invalid_sums=False, sigma_noise=None, jitter=None, lindisp=True, want_z=False):
    """rays (n*Bp, 8), z_samp (n*Bp, K) -> dict of fresh tensors (bts_render_fwd).  want_saved adds the two per-sample
    activations the backward needs (sigma_raw, trans); want_invalid_sums the per-ray reductions the loss' invalid-ray policies need
    (invalid_wsum = sum_k weights * invalid, invalid_any = max_k invalid, (n*Bp, nv) each) -- with them a training step can leave
    weights / invalid / rgb_samps unrequested.
    z_samp=None with ``jitter`` (n*Bp, K) in [0, 1): NeRFRenderer.sample_coarse runs inside the kernel (BtsRenderArgs.jitter, ``lindisp``
    as the renderer's flag); the depths come back as out["z_samp"] when ``want_z`` (bit-identical to ``sample_coarse(rays, jitter)``)."""
    if z_samp is None:
        if jitter is None:
            raise BtsNativeError("render_fwd needs z_samp or jitter")
        if ft.proj_nhwc is None:
            raise BtsNativeError("in-kernel sampling (jitter) needs the projected feature map")
        _req(jitter, "jitter")
    else:
        _req(z_samp, "z_samp")
        jitter = None
    B, K = (z_samp if z_samp is not None else jitter).shape
    _req(rays, "rays", (B, 8)), _req(mlp_params.detach(), "mlp_params", (ft.spec.mlp_param_count(),))
    if B % ft.n != 0:
        raise BtsNativeError(f"{B} rays do not split evenly over n={ft.n} samples")
    _check_partial(ft, rays, z_samp if z_samp is not None else jitter)
    dev, nv = rays.device, ft.nv

    def new(*shape):
        return torch.empty(shape, device=dev, dtype=torch.float32)

    if ft.mlp_color and want_invalid_sums:
        raise BtsNativeError("render_fwd: MLP-predicted colour produces no invalid_wsum / invalid_any (request weights and invalid instead)")
    multi = isinstance(ft, MultiViewField)
    if multi and want_invalid_sums:
        raise BtsNativeError("render_fwd: merged encoder views produce no invalid_wsum / invalid_any (request weights and invalid instead)")
    outs = dict(rgb=new(B, nv * 3), depth=new(B), weights=new(B, K) if want_weights else None,
                alphas=new(B, K) if want_alphas else None, invalid=new(B, K, nv) if want_invalid else None,
                rgb_samps=new(B, K, nv * 3) if want_rgb_samps else None, sigma_raw=new(B, K) if want_saved else None,
                trans=new(B, K) if want_saved else None, invalid_wsum=new(B, nv) if want_invalid_sums else None,
                invalid_any=new(B, nv) if want_invalid_sums else None,
                z_samp=new(B, K) if (z_samp is None and want_z) else None)
    args = _render_args(ft, rays, z_samp, hard_alpha_cap, white_bkgd, outs, sigma_noise, jitter, lindisp)
    if multi:
        mv = ft.struct(mlp_params)
        _lib.check(_lib.load().bts_render_fwd_multi_view(C.byref(mv), C.byref(args), _stream(rays)), "bts_render_fwd_multi_view")
    else:
        cfg, tens = ft.cfg(), ft.tensors(mlp_params)
        fn = "bts_render_fwd_mlp_color" if ft.mlp_color else "bts_render_fwd"
        _lib.check(getattr(_lib.load(), fn)(C.byref(cfg), C.byref(tens), C.byref(args), _stream(rays)), fn)
    if z_samp is not None:
        outs["z_samp"] = z_samp
    return outs


def _check_partial(ft: "FieldTensors", rays, samples, what="render"):
    """A map projected for one sample set (FieldTensors.partial) serves that set and nothing else."""
    if ft.partial is None:
        return
    if samples is None or rays is None:
        raise BtsNativeError(f"{what}: this field's projected map holds only the tiles ONE render's samples read (native_field(sampled=...)); "
                             "field queries need the full map: call net.native_field() without `sampled`")
    if (rays.data_ptr(), rays.shape[0]) != ft.partial[:2]:
        raise BtsNativeError(f"{what}: the projected map of this field was built for another ray set (sparse projection, native_field(sampled=...))")


def _render_bwd_checks(z_samp, sigma_raw, trans, g_rgb, g_depth, g_weights, g_alphas):
    """What every render backward checks first: the upstream gradients and the forward's saved state."""
    B, K = z_samp.shape
    for name, g in (("g_rgb", g_rgb), ("g_depth", g_depth), ("g_weights", g_weights), ("g_alphas", g_alphas)):
        if g is not None:
            _req(g, name)
    _req(sigma_raw, "sigma_raw", (B, K)), _req(trans, "trans", (B, K))


def _render_bwd_structs(ft, rays, z_samp, sigma_raw, trans, hard_alpha_cap, white_bkgd, g_rgb, g_depth, g_weights, g_alphas, need_mlp, need_empty,
                        rgb_samps, sigma_noise, d_proj=None, tiles=None):
    """Behind the caller's map gradients: zeroed d_mlp_params and d_empty_proj, the rgb_samps check, BtsRenderArgs and BtsRenderGrads
    (d_proj, tiles: the single map of bts_render_bwd).  Returns (args, grads, d_mlp, d_empty)."""
    B, K = z_samp.shape
    dev = rays.device
    d_mlp = torch.zeros(ft.spec.mlp_param_count(), device=dev, dtype=torch.float32) if need_mlp else None
    d_empty = torch.zeros(ft.spec.d_hidden, device=dev, dtype=torch.float32) if need_empty else None
    if rgb_samps is not None:
        _req(rgb_samps, "rgb_samps", (B, K, ft.nv * 3))
    args = _render_args(ft, rays, z_samp, hard_alpha_cap, white_bkgd, dict(sigma_raw=sigma_raw, trans=trans, rgb_samps=rgb_samps), sigma_noise)
    grads = BtsRenderGrads(g_rgb=_addr(g_rgb), g_depth=_addr(g_depth), g_weights=_addr(g_weights), g_alphas=_addr(g_alphas),
                           d_proj_nhwc=_addr(d_proj), d_mlp_params=_addr(d_mlp), d_empty_proj=_addr(d_empty), d_proj_tiles=_addr(tiles))
    return args, grads, d_mlp, d_empty


def render_bwd(ft: FieldTensors, mlp_params, rays, z_samp, sigma_raw, trans, *, hard_alpha_cap, g_rgb=None, g_depth=None,
               g_weights=None, g_alphas=None, need_proj=True, need_mlp=True, need_empty=False, white_bkgd=False, rgb_samps=None,
               sigma_noise=None, proj_grad=None):
    """Returns (d_proj_nhwc | None, d_mlp_params | None, d_empty_proj | None) (bts_render_bwd).  ``proj_grad`` = (d_proj, tiles): add
    into THIS d_proj (the caller vouches that it is zero wherever ``tiles`` is) and flag the 64-texel tiles that received something
    (BtsRenderGrads.d_proj_tiles) -- no fill of a map-sized tensor."""
    _render_bwd_checks(z_samp, sigma_raw, trans, g_rgb, g_depth, g_weights, g_alphas)
    dev = rays.device
    tiles = None
    if need_proj and proj_grad is not None:
        d_proj, tiles = proj_grad
        _req(d_proj, "proj_grad[0]", tuple(ft.proj_nhwc.shape))
    else:
        d_proj = torch.zeros(ft.proj_nhwc.shape, device=dev, dtype=torch.float32) if need_proj else None
    args, grads, d_mlp, d_empty = _render_bwd_structs(ft, rays, z_samp, sigma_raw, trans, hard_alpha_cap, white_bkgd, g_rgb, g_depth, g_weights,
                                                      g_alphas, need_mlp, need_empty, rgb_samps, sigma_noise, d_proj, tiles)
    cfg, tens = ft.cfg(), ft.tensors(mlp_params)
    lib = _lib.load()
    if ft.mlp_color:
        ws_bytes = lib.bts_render_bwd_mlp_color_workspace(C.byref(cfg), C.byref(args))
        ws = _workspace(dev, int(ws_bytes))
        _lib.check(lib.bts_render_bwd_mlp_color(C.byref(cfg), C.byref(tens), C.byref(args), C.byref(grads), _ptr(ws), ws_bytes, _stream(rays)),
                   "bts_render_bwd_mlp_color")
        return d_proj, d_mlp, d_empty
    ws_bytes = lib.bts_render_bwd_workspace(C.byref(cfg), C.byref(args))
    ws = _workspace(dev, int(ws_bytes))
    _lib.check(lib.bts_render_bwd(C.byref(cfg), C.byref(tens), C.byref(args), C.byref(grads), _ptr(ws), ws_bytes, _stream(rays)),
               "bts_render_bwd")
    return d_proj, d_mlp, d_empty


def render_bwd_multi_view(ft: MultiViewField, mlp_params, rays, z_samp, sigma_raw, trans, *, hard_alpha_cap, g_rgb=None, g_depth=None,
                          g_weights=None, g_alphas=None, need_proj=None, need_mlp=True, need_empty=False, white_bkgd=False, rgb_samps=None,
                          sigma_noise=None):
    """Returns ([d_proj_nhwc | None per encoder view], d_mlp_params | None, d_empty_proj | None) (bts_render_bwd_multi_view); ``need_proj``:
    one flag per view (None: every view)."""
    _render_bwd_checks(z_samp, sigma_raw, trans, g_rgb, g_depth, g_weights, g_alphas)
    dev, V = rays.device, len(ft.views)
    need_proj = [True] * V if need_proj is None else list(need_proj)
    d_projs = [torch.zeros(v.proj_nhwc.shape, device=dev, dtype=torch.float32) if need else None for v, need in zip(ft.views, need_proj)]
    args, grads, d_mlp, d_empty = _render_bwd_structs(ft, rays, z_samp, sigma_raw, trans, hard_alpha_cap, white_bkgd, g_rgb, g_depth, g_weights,
                                                      g_alphas, need_mlp, need_empty, rgb_samps, sigma_noise)
    maps = (C.c_void_p * V)(*[_addr(d) for d in d_projs])
    mv, lib = ft.struct(mlp_params), _lib.load()
    ws_bytes = lib.bts_render_bwd_multi_view_workspace(C.byref(mv), C.byref(args))
    ws = _workspace(dev, int(ws_bytes))
    _lib.check(lib.bts_render_bwd_multi_view(C.byref(mv), C.byref(args), C.byref(grads), maps, None, _ptr(ws), ws_bytes, _stream(rays)),
               "bts_render_bwd_multi_view")
    return d_projs, d_mlp, d_empty


_WS = {}
WORKSPACE_CACHE_LIMIT = 256 << 20   # bytes: larger scratch is allocated per call and goes back to torch's caching allocator


def _workspace(dev, n_bytes):
    """Scratch of the backward (what its passes hand each other: 20 B per sample on the bit path, 4 + 4 d_hidden B per sample on the row
    path).  Buffers up to WORKSPACE_CACHE_LIMIT are kept per device and stream, grown on demand and reused -- the contents need no
    initialisation and every use is ordered on the stream; anything larger is a plain torch allocation of this call, so that an
    occasional huge backward does not pin its scratch for the life of the process (release_workspace() drops the kept ones too)."""
    if n_bytes > WORKSPACE_CACHE_LIMIT:
        return torch.empty(n_bytes // 4 + 1, device=dev, dtype=torch.float32)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() * 4 < n_bytes + 4:
        buf = torch.empty(n_bytes // 4 + 1, device=dev, dtype=torch.float32)
        _WS[key] = buf
    return buf


def release_workspace():
    """Drops the cached backward scratch (e.g. when a process switches from training to evaluation)."""
    _WS.clear()


def field_query(ft: FieldTensors, mlp_params: torch.Tensor, xyz: torch.Tensor, only_density: bool = False):
    """xyz (n, P, 3) -> rgb (n,P,nv*3) | None, invalid (n,P,nv or 1), sigma (n,P,1)  (bts_field_query)."""
    n, P, _ = xyz.shape
    _req(xyz, "xyz", (ft.n, P, 3))
    _check_partial(ft, None, None, "field_query")
    dev = xyz.device
    if isinstance(ft, MultiViewField) and only_density:
        raise NotImplementedError("only_density with several encoder views: the reference itself fails here (models_bts.py:281-284)")
    sigma = torch.empty((n, P, 1), device=dev, dtype=torch.float32)
    if isinstance(ft, MultiViewField):
        rgb = torch.empty((n, P, ft.nv * 3), device=dev, dtype=torch.float32)
        invalid = torch.empty((n, P, ft.nv), device=dev, dtype=torch.float32)
        mv = ft.struct(mlp_params)
        _lib.check(_lib.load().bts_field_query_multi_view(C.byref(mv), _ptr(xyz), P, _ptr(rgb), _ptr(invalid), _ptr(sigma), _stream(xyz)),
                   "bts_field_query_multi_view")
        return rgb, invalid, sigma
    if ft.mlp_color:
        # sample_color=False (models_bts.py:315-338): rgb (n, P, 3) from the MLP, zeros with only_density (:336); invalid (n, P, 1)
        rgb = torch.empty((n, P, 3), device=dev, dtype=torch.float32)
        invalid = torch.empty((n, P, 1), device=dev, dtype=torch.float32)
        cfg, tens = ft.cfg(), ft.tensors(mlp_params)
        _lib.check(_lib.load().bts_field_query_mlp_color(C.byref(cfg), C.byref(tens), _ptr(xyz), P, int(only_density), _ptr(rgb), _ptr(invalid),
                                                         _ptr(sigma), _stream(xyz)), "bts_field_query_mlp_color")
        return rgb, invalid, sigma
    nv = 0 if only_density else ft.nv
    rgb = torch.empty((n, P, nv * 3), device=dev, dtype=torch.float32) if nv else None
    invalid = torch.empty((n, P, max(nv, 1)), device=dev, dtype=torch.float32)
    if nv == 0 and not only_density:  # no colour views: invalid is the feature-frustum test only
        only_density = True
    cfg, tens = ft.cfg(), ft.tensors(mlp_params)
    _lib.check(_lib.load().bts_field_query(C.byref(cfg), C.byref(tens), _ptr(xyz), P, int(only_density), _ptr(rgb), _ptr(invalid),
                                           _ptr(sigma), _stream(xyz)), "bts_field_query")
    return rgb, invalid, sigma


# --------------------------------------------------------------------------------------------------------------
# patch colours (image_processor {type: patch}): 27 channels per render view from the render's weights
# --------------------------------------------------------------------------------------------------------------
PATCH_COLOR_MESSAGE = ("patch colours (native_patch_color: a 27-channel images_alt) are rendered by the entry-by-entry path only: the render "
                       "kernels, then bts_patch_color_fwd / _bwd on their weights")


def _patch_color_struct(ft, patch, rays=None, z_samp=None, weights=None, white_bkgd=False, rgb=None, rgb_samps=None):
    if ft.imgs_nhwc4 is None or ft.nv < 1:
        raise BtsNativeError("patch colours need the packed colour frames and the render cameras (nv >= 1)")
    B, K = z_samp.shape if z_samp is not None else (0, 0)
    return _lib.BtsPatchColor(n=ft.n, nv=ft.nv, H=ft.H, W=ft.W, K=K, patch=int(patch), white_bkgd=int(bool(white_bkgd)), reserved_=0,
                              rays_per_sample=B // ft.n, rays=_addr(rays), z_samp=_addr(z_samp), weights=_addr(weights),
                              imgs_nhwc4=_addr(ft.imgs_nhwc4), K_r=_addr(ft.K_r), w2c_r=_addr(ft.w2c_r), rgb=_addr(rgb), rgb_samps=_addr(rgb_samps))


def _patch_color_rays(ft, rays, z_samp):
    B, K = z_samp.shape
    _req(rays, "rays", (B, 8)), _req(z_samp, "z_samp")
    if B % ft.n != 0:
        raise BtsNativeError(f"{B} rays do not split evenly over n={ft.n} samples")
    return B, K


def patch_color_fwd(ft: FieldTensors, rays, z_samp, weights, *, white_bkgd=False, want_rgb_samps=False, patch=3):
    """rays (B, 8), z_samp / weights (B, K) of a render of ``ft`` -> rgb (B, nv * 27), rgb_samps (B, K, nv * 27) | None
    (bts_patch_color_fwd): rgb = sum_k weights * the double-clamp colours (+ 1 - sum weights with white_bkgd)."""
    B, K = _patch_color_rays(ft, rays, z_samp)
    _req(weights, "weights", (B, K))
    ch = ft.nv * _lib.BTS_PATCH_COLOR_CHANNELS
    rgb = torch.empty((B, ch), device=rays.device, dtype=torch.float32)
    rgb_samps = torch.empty((B, K, ch), device=rays.device, dtype=torch.float32) if want_rgb_samps else None
    a = _patch_color_struct(ft, patch, rays, z_samp, weights, white_bkgd, rgb, rgb_samps)
    _lib.check(_lib.load().bts_patch_color_fwd(C.byref(a), _stream(rays)), "bts_patch_color_fwd")
    return rgb, rgb_samps


def patch_color_bwd(ft: FieldTensors, rays, z_samp, g_rgb, *, white_bkgd=False, patch=3):
    """g_rgb (B, nv * 27) -> g_weights (B, K) = sum_{v, ch} g_rgb * colour (- sum g_rgb with white_bkgd)  (bts_patch_color_bwd)."""
    B, K = _patch_color_rays(ft, rays, z_samp)
    _req(g_rgb, "g_rgb", (B, ft.nv * _lib.BTS_PATCH_COLOR_CHANNELS))
    g_weights = torch.empty((B, K), device=rays.device, dtype=torch.float32)
    a = _patch_color_struct(ft, patch, rays, z_samp, None, white_bkgd)
    _lib.check(_lib.load().bts_patch_color_bwd(C.byref(a), _ptr(g_rgb), _ptr(g_weights), _stream(rays)), "bts_patch_color_bwd")
    return g_weights


def patch_color_query(ft: FieldTensors, xyz, patch=3):
    """xyz (n, P, 3) -> the points' colours in every render view, (n, P, nv * 27)  (bts_patch_color_query)."""
    n, P, _ = xyz.shape
    _req(xyz, "xyz", (ft.n, P, 3))
    rgb = torch.empty((n, P, ft.nv * _lib.BTS_PATCH_COLOR_CHANNELS), device=xyz.device, dtype=torch.float32)
    a = _patch_color_struct(ft, patch)
    _lib.check(_lib.load().bts_patch_color_query(C.byref(a), _ptr(xyz), P, _ptr(rgb), _stream(xyz)), "bts_patch_color_query")
    return rgb


class PatchColorFunction(torch.autograd.Function):
    """The 27-channel colours behind a render, chained after RenderFunction.  Differentiable input: ``weights`` (the render's);
    differentiable output: rgb (B, nv * 27).  rgb_samps (B, K, nv * 27, or empty) carries no gradient.  Nothing per sample is saved: the
    backward forms the taps again from rays and z_samp."""

    @staticmethod
    def forward(ctx, weights, ft: FieldTensors, rays, z_samp, white_bkgd, want_rgb_samps):
        ctx.set_materialize_grads(False)
        rgb, rgb_samps = patch_color_fwd(ft, rays, z_samp, weights.detach().contiguous(), white_bkgd=white_bkgd, want_rgb_samps=want_rgb_samps,
                                         patch=ft.patch)
        ctx.ft, ctx.white_bkgd = ft, white_bkgd
        ctx.save_for_backward(rays, z_samp)
        rs = rgb_samps if want_rgb_samps else rays.new_empty(0)
        ctx.mark_non_differentiable(rs)
        return rgb, rs

    @staticmethod
    def backward(ctx, g_rgb, _g_rs):
        if g_rgb is None:
            return (None,) * 6
        rays, z_samp = ctx.saved_tensors
        return (patch_color_bwd(ctx.ft, rays, z_samp, g_rgb.contiguous(), white_bkgd=ctx.white_bkgd, patch=ctx.ft.patch),) + (None,) * 5


def occupancy_profile(ft: FieldTensors, mlp_params: torch.Tensor, xyz: torch.Tensor, levels: int, threshold: float = 8.0,
                      only_density: bool = False, want_sigma: bool = False):
    """xyz (n, levels * columns, 3): a dense grid of query points, the vertical level slowest -> profile (n, columns)
    [, sigma (n, levels * columns)]  (bts_occupancy_profile: render_profile of scripts/inference_setup.py in one pass)."""
    n, P, _ = xyz.shape
    _req(xyz, "xyz", (ft.n, P, 3))
    if isinstance(ft, MultiViewField):
        raise BtsNativeError("occupancy_profile: not available for a field with more than one encoder view; use field_query")
    if ft.mlp_color:
        raise BtsNativeError("occupancy_profile: not available for MLP-predicted colour (sample_color=False); use field_query")
    if levels <= 0 or P % levels:
        raise BtsNativeError(f"{P} points are not {levels} whole levels")
    _check_partial(ft, None, None, "occupancy_profile")
    cols = P // levels
    profile = torch.empty((n, cols), device=xyz.device, dtype=torch.float32)
    sigma = torch.empty((n, P), device=xyz.device, dtype=torch.float32) if want_sigma else None
    cfg, tens = ft.cfg(nv=0 if only_density else None), ft.tensors(mlp_params)
    _lib.check(_lib.load().bts_occupancy_profile(C.byref(cfg), C.byref(tens), _ptr(xyz), levels, cols, float(threshold), int(only_density),
                                                 _ptr(profile), _ptr(sigma), _stream(xyz)), "bts_occupancy_profile")
    return (profile, sigma) if want_sigma else profile


DEPTH_SCALING_MODES = {None: 0, "median": 1, "l2": 2}


def depth_metrics(pred: torch.Tensor, gt: torch.Tensor, depth_scaling=None, clamp=(1e-3, 80.0), out=None, counts=None):
    """pred (B, H, W) z-depth, gt (B, Hg, Wg) with 0 = no measurement -> rows (B, 12): abs_rel sq_rel rmse rmse_log a1 a2 a3 scale shift
    n_metric n_scale 0 -- compute_depth_metrics of models/bts/evaluator.py:96-151 per frame (bts_depth_metrics).  ``out`` / ``counts``:
    the caller's (B, 12) float32 / (B, 5) int32 buffers (n_metric, n_scale and the three threshold counts as integers).  The workspace is
    the cached per-stream scratch of this module; nothing synchronises."""
    _req(pred, "depth_pred"), _req(gt, "depth_gt")
    if pred.dim() != 3 or gt.dim() != 3 or pred.shape[0] != gt.shape[0]:
        raise BtsNativeError(f"depth_metrics: expected (B, H, W) and (B, Hg, Wg), got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if depth_scaling not in DEPTH_SCALING_MODES:
        raise BtsNativeError(f"depth_scaling: expected None, 'median' or 'l2', got {depth_scaling!r}")
    if pred.device != gt.device:
        raise BtsNativeError(f"depth_pred on {pred.device}, depth_gt on {gt.device}")
    B, H, W = pred.shape
    Hg, Wg = gt.shape[1:]
    mode = DEPTH_SCALING_MODES[depth_scaling]
    if out is None:
        out = torch.empty((B, _lib.BTS_DEPTH_METRICS_ROW), device=pred.device, dtype=torch.float32)
    else:
        _req(out, "out", (B, _lib.BTS_DEPTH_METRICS_ROW))
    if counts is not None:
        _req_as(counts, "counts", torch.int32, (B, 5))
    lib = _lib.load()
    ws_bytes = int(lib.bts_depth_metrics_workspace(B, Hg, Wg, mode))
    ws = _workspace(pred.device, max(ws_bytes, 16))
    args = _lib.BtsDepthMetrics(pred=pred.data_ptr(), H=H, W=W, gt=gt.data_ptr(), Hg=Hg, Wg=Wg, B=B, mode=mode, clamp_lo=float(clamp[0]),
                                clamp_hi=float(clamp[1]), metrics=out.data_ptr(), counts=_addr(counts))
    _lib.check(lib.bts_depth_metrics(C.byref(args), _ptr(ws), ws_bytes, _stream(pred)), "bts_depth_metrics")
    return out


def lidar_depth(points: torch.Tensor, offsets, P: torch.Tensor, size, convention, eigen_depth=False, out=None, max_blocks=0):
    """points (N, 4) float32, the B Velodyne clouds concatenated; ``offsets``: B + 1 host integers (cloud f is
    ``points[offsets[f]:offsets[f + 1]]``); P (3, 4) float32 or float64 -> the ground-truth depth maps (B, H, W) in P's dtype --
    load_depth of datasets/kitti_raw/kitti_raw_dataset.py:256-302 (``convention="kitti_raw"``, with its ``eigen_depth``) or of
    datasets/kitti_360/kitti_360_dataset.py:505-539 (``"kitti_360"``) per cloud (bts_lidar_depth).  ``out``: the caller's (B, H, W)
    buffer.  ``max_blocks``: a cap on the points pass's grid (tests).  The workspace is the cached per-stream scratch of this module;
    nothing synchronises."""
    if not isinstance(convention, str) or convention not in _lib.BTS_LIDAR_DEPTH_CONVENTIONS:
        raise ValueError(f"convention: expected 'kitti_raw' or 'kitti_360', got {convention!r}")
    if eigen_depth and convention != "kitti_raw":
        raise ValueError("eigen_depth: the Eigen crop is kitti_raw's; kitti_360's load_depth has none")
    try:
        H, W = (int(s) for s in size)
    except (TypeError, ValueError):
        raise ValueError(f"size: expected (H, W), got {size!r}") from None
    if not isinstance(P, torch.Tensor) or P.dtype not in (torch.float32, torch.float64):
        raise BtsNativeError(f"P: expected a float32 or float64 tensor, got {getattr(P, 'dtype', type(P).__name__)}")
    _req_as(P, "P", P.dtype, (3, 4))
    _req(points, "points")
    if points.dim() != 2 or points.shape[1] != 4:
        raise BtsNativeError(f"points: expected shape (N, 4), got {tuple(points.shape)}")
    if points.device != P.device:
        raise BtsNativeError(f"points on {points.device}, P on {P.device}")
    offs = [int(o) for o in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
    B = len(offs) - 1
    if B < 1 or offs[0] != 0 or offs[-1] != points.shape[0] or any(b < a for a, b in zip(offs, offs[1:])):
        raise ValueError(f"offsets: expected B + 1 non-decreasing integers from 0 to N={points.shape[0]}, got {offs}")
    if H <= 0 or W <= 0:
        raise ValueError(f"size: expected a positive (H, W), got {(H, W)}")
    if out is None:
        out = torch.empty((B, H, W), device=points.device, dtype=P.dtype)
    else:
        _req_as(out, "out", P.dtype, (B, H, W))
    lib = _lib.load()
    p64 = int(P.dtype == torch.float64)
    ws_bytes = int(lib.bts_lidar_depth_workspace(B, H, W, p64))
    ws = _workspace(points.device, max(ws_bytes, 16))
    c_offs = (C.c_int64 * (B + 1))(*offs)
    args = _lib.BtsLidarDepth(points=_addr(points) if points.shape[0] else None, offsets=c_offs, P=P.data_ptr(), B=B, H=H, W=W,
                              convention=_lib.BTS_LIDAR_DEPTH_CONVENTIONS[convention], eigen_depth=int(bool(eigen_depth)), p_fp64=p64,
                              max_blocks=int(max_blocks), depth=out.data_ptr())
    _lib.check(lib.bts_lidar_depth(C.byref(args), _ptr(ws), ws_bytes, _stream(points)), "bts_lidar_depth")
    return out


def nvs_crop_box(eval_resolution):
    """The 5 % crop of evaluator_nvs.py:158-161 at ``eval_resolution = (h, w)``: (y0, y1, x0, x1), the reference's own expressions on
    Python floats; bts_nvs_metrics takes the box from here and derives none of its own."""
    h, w = int(eval_resolution[0]), int(eval_resolution[1])
    return int(math.ceil(0.05 * h)), int(math.floor(0.95 * h)), int(math.ceil(0.05 * w)), int(math.floor(0.95 * w))


def nvs_metrics(pred: torch.Tensor, gt: torch.Tensor, eval_resolution, out=None):
    """pred, gt (B, H, W, 3) float32 VIEWS of any strides (a slice of the render's output, a permuted channel-planar image) -> rows
    (B, 8) float64: ssim psnr mse ssim_c0 ssim_c1 ssim_c2 n_interior n_crop -- the image half of compute_nvs_metrics of
    models/bts/evaluator_nvs.py:141-178 per frame (bts_nvs_metrics): nearest resize to ``eval_resolution``, the 5 % crop, skimage's
    SSIM (7 x 7 uniform window, fp64) and PSNR.  ``out``: the caller's (B, 8) float64 buffer.  Nothing is copied and nothing synchronises."""
    _req_as(pred, "rgb_pred", torch.float32, contiguous=False), _req_as(gt, "rgb_gt", torch.float32, contiguous=False)
    if pred.dim() != 4 or pred.shape[-1] != 3 or pred.shape != gt.shape:
        raise BtsNativeError(f"nvs_metrics: expected two (B, H, W, 3) views of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if pred.device != gt.device:
        raise BtsNativeError(f"rgb_pred on {pred.device}, rgb_gt on {gt.device}")
    if len(eval_resolution) != 2:
        raise BtsNativeError(f"eval_resolution: (height, width) expected, got {eval_resolution!r}")
    B, H, W, _ = pred.shape
    He, We = int(eval_resolution[0]), int(eval_resolution[1])
    y0, y1, x0, x1 = nvs_crop_box((He, We))
    if out is None:
        out = torch.empty((B, _lib.BTS_NVS_METRICS_ROW), device=pred.device, dtype=torch.float64)
    elif _req_as(out, "out", torch.float64, (B, _lib.BTS_NVS_METRICS_ROW)).device != pred.device:
        raise BtsNativeError(f"out on {out.device}, rgb_pred on {pred.device}")
    lib = _lib.load()
    ws_bytes = int(lib.bts_nvs_metrics_workspace(B, He, We))
    ws = _workspace(pred.device, max(ws_bytes, 16))
    ps, gs = pred.stride(), gt.stride()
    args = _lib.BtsNvsMetrics(pred=pred.data_ptr(), pred_sb=ps[0], pred_sy=ps[1], pred_sx=ps[2], pred_sc=ps[3], gt=gt.data_ptr(), gt_sb=gs[0],
                              gt_sy=gs[1], gt_sx=gs[2], gt_sc=gs[3], B=B, H=H, W=W, He=He, We=We, y0=y0, y1=y1, x0=x0, x1=x1,
                              data_range=1.0, metrics=out.data_ptr())
    _lib.check(lib.bts_nvs_metrics(C.byref(args), _ptr(ws), ws_bytes, _stream(pred)), "bts_nvs_metrics")
    return out


# --------------------------------------------------------------------------------------------------------------
# novel-view frames and colour-mapped depth (csrc/bts_frames.hip; the host mirrors live in novel_views.py)
# --------------------------------------------------------------------------------------------------------------
def _req_canvas(canvas, B, h, w, row0, col0, what):
    if not isinstance(canvas, torch.Tensor) or canvas.dim() != 4 or canvas.shape[0] != B or canvas.shape[3] != 3:
        raise BtsNativeError(f"canvas: a ({B}, Hc, Wc, 3) uint8 tensor expected")
    _req_as(canvas, "canvas", torch.uint8)
    Hc, Wc = int(canvas.shape[1]), int(canvas.shape[2])
    if row0 < 0 or col0 < 0 or row0 + h > Hc or col0 + w > Wc:
        raise BtsNativeError(f"the {what} panel ({h} x {w} at ({row0}, {col0})) leaves the {Hc} x {Wc} canvas")
    return Hc, Wc


def colorize(x: torch.Tensor, N: int, lut_f64=None, lut_u8=None, norm: bool = False, want_f64: bool = True, canvas=None, row0: int = 0,
             col0: int = 0):
    """x (B, h, w) float32 -> matplotlib's colour map per pixel (bts_colorize): a fresh (B, h, w, 3) float64 tensor from ``lut_f64``
    (N + 3, 3) when ``want_f64``, and / or the bytes of ``lut_u8`` (N + 3, 3) into ``canvas`` (B, Hc, Wc, 3) at (row0, col0).  ``norm``:
    (x - min) / (max - min) per image first.  Nothing synchronises."""
    _req(x, "x")
    if x.dim() != 3:
        raise BtsNativeError(f"x: (B, h, w) expected, got {tuple(x.shape)}")
    B, h, w = (int(s) for s in x.shape)
    if B == 0 or h * w == 0:
        raise BtsNativeError("x: an empty image")
    dev, out, Hc, Wc = x.device, None, 0, 0
    if want_f64:
        _req_as(lut_f64, "lut_f64", torch.float64, (N + 3, 3))
        out = torch.empty((B, h, w, 3), device=dev, dtype=torch.float64)
    if canvas is not None:
        _req_as(lut_u8, "lut_u8", torch.uint8, (N + 3, 3))
        Hc, Wc = _req_canvas(canvas, B, h, w, row0, col0, "colour")
    if out is None and canvas is None:
        raise BtsNativeError("colorize: neither the float64 output nor a canvas was requested")
    scratch = _workspace(dev, B * _lib.BTS_FRAMES_PARTIALS * 3 * 4) if norm else None
    _lib.check(_lib.load().bts_colorize(_ptr(x), B, h, w, int(bool(norm)), int(N), _ptr(lut_f64) if want_f64 else None,
                                        _ptr(lut_u8) if canvas is not None else None, _ptr(scratch), _ptr(out), _ptr(canvas), Hc, Wc, int(row0),
                                        int(col0), _stream(x)), "bts_colorize")
    return out


def pack_u8(x: torch.Tensor, canvas: torch.Tensor, row0: int = 0, col0: int = 0, scale: float = 1.0, shift: float = 0.0):
    """x (B, h, w, 3) float32 VIEW of any strides (a permuted channel-planar image) -> uint8 of x * scale + shift into ``canvas``
    (B, Hc, Wc, 3) at (row0, col0) (bts_pack_u8)."""
    _req_as(x, "x", torch.float32, contiguous=False)
    if x.dim() != 4 or x.shape[-1] != 3 or x.numel() == 0:
        raise BtsNativeError(f"x: a non-empty (B, h, w, 3) view expected, got {tuple(x.shape)}")
    B, h, w, _ = (int(s) for s in x.shape)
    Hc, Wc = _req_canvas(canvas, B, h, w, row0, col0, "image")
    st = x.stride()
    _lib.check(_lib.load().bts_pack_u8(_ptr(x), st[0], st[1], st[2], st[3], B, h, w, float(scale), float(shift), _ptr(canvas), Hc, Wc, int(row0),
                                       int(col0), _stream(x)), "bts_pack_u8")
    return canvas


def novel_views(ft: Optional["FieldTensors"], mlp_params, a: "_lib.BtsNovelViews", stream):
    """One chunk of novel views (bts_novel_views); ``a`` is filled by novel_views.py.  ``ft`` None: finish_only."""
    if ft is None:
        _lib.check(_lib.load().bts_novel_views(None, None, C.byref(a), stream), "bts_novel_views")
        return
    _check_partial(ft, None, None, "novel_views")
    cfg, tens = ft.cfg(), ft.tensors(mlp_params)
    _lib.check(_lib.load().bts_novel_views(C.byref(cfg), C.byref(tens), C.byref(a), stream), "bts_novel_views")


def train_vis(imgs, rgb, depths, alphas, invalid, z_near, z_far, N: int, lut_f64, fields: bool = False):
    """The trainer's visualisation panels (bts_train_vis, csrc/bts_train_vis.hip) for batch element 0: ``imgs`` a list of >= T tensors
    ``(3, h, w)``, ``rgb (v, h, w, nv, 3)``, ``depths`` a list of S ``(v, h, w)``, ``alphas (v, h, w, K)``, ``invalid (v, h, w, K, nv)``,
    all contiguous float32 on one GPU and read where they lie; ``lut_f64 (N + 3, 3)``; ``z_near`` / ``z_far`` two numbers, or two
    tensors on that GPU (the trainer's: read by the kernel, no ``.item()``).  T = min(v, 6).  -> dict of the eight panels
    (``recon_depth`` as ``(S, T, 3, h, w)``), plus the six ``f_*`` fields with ``fields``.  Nothing synchronises, the inputs are not
    written."""
    _req(alphas, "alphas")
    if alphas.dim() != 4:
        raise BtsNativeError(f"alphas: (v, h, w, K) expected, got {tuple(alphas.shape)}")
    v, h, w, K = (int(s) for s in alphas.shape)
    T = min(v, _lib.BTS_TRAIN_VIS_MAX_FRAMES)
    _req(invalid, "invalid")
    if invalid.dim() != 5 or tuple(invalid.shape[:4]) != (v, h, w, K):
        raise BtsNativeError(f"invalid: ({v}, {h}, {w}, {K}, nv) expected, got {tuple(invalid.shape)}")
    nv = int(invalid.shape[4])
    _req(rgb, "rgb", (v, h, w, nv, 3))
    if len(imgs) < T:
        raise BtsNativeError(f"imgs: {T} frames expected, got {len(imgs)}")
    if not 1 <= len(depths) <= _lib.BTS_MAX_SCALES:
        raise BtsNativeError(f"depths: 1 .. {_lib.BTS_MAX_SCALES} scales expected, got {len(depths)}")
    S, dev = len(depths), alphas.device
    _req_as(lut_f64, "lut_f64", torch.float64, (N + 3, 3))
    a = _lib.BtsTrainVis(T=T, v=v, h=h, w=w, K=K, nv=nv, S=S, lut_N=int(N), rgb=_addr(rgb), alphas=_addr(alphas), invalid=_addr(invalid),
                         lut=_addr(lut_f64))
    z_pair = None
    if isinstance(z_near, torch.Tensor) or isinstance(z_far, torch.Tensor):
        z_pair = torch.stack([torch.as_tensor(z, device=dev).detach().reshape(()).float() for z in (z_near, z_far)])
        a.z_near_far = z_pair.data_ptr()
    else:
        a.z_near, a.z_far = float(z_near), float(z_far)
    for i in range(T):
        a.imgs[i] = _addr(_req(imgs[i], f"imgs[{i}]", (3, h, w)))
    for i, d in enumerate(depths):
        a.depth[i] = _addr(_req(d, f"depth[{i}]", (v, h, w)))
    for t in list(imgs[:T]) + list(depths) + [rgb, invalid, lut_f64]:
        if t.device != dev:
            raise BtsNativeError(f"every input must live on {dev} (got {t.device})")
    need = int(_lib.load().bts_train_vis_workspace(T, h, w, K))
    if need == 0:
        raise BtsNativeError(f"train_vis: T={T}, h={h}, w={w}, K={K} is outside the envelope (K in [2, 256], h and w at most 8192)")
    f32 = dict(device=dev, dtype=torch.float32)
    out = dict(input_im=torch.empty((T, 3, h, w), **f32), recon_im=torch.empty((T, 3, h, w), **f32),
               recon_depth=torch.empty((S, T, 3, h, w), **f32), depth_profile=torch.empty((3 * T, 3, K, w), **f32),
               ray_entropy=torch.empty((T, 3, h, w), **f32), alpha_sum=torch.empty((T, 3, h, w), **f32),
               recon_mse=torch.empty((T, 3, h, w), **f32), invalids=torch.empty((T, 3, h, w), **f32))
    if fields:
        out.update(f_depth=torch.empty((S, T, h, w), **f32), f_profile=torch.empty((3 * T, K, w), **f32), f_entropy=torch.empty((T, h, w), **f32),
                   f_alpha_sum=torch.empty((T, h, w), **f32), f_mse=torch.empty((T, h, w), **f32), f_invalid=torch.empty((T, h, w), **f32))
    for k, t in out.items():
        setattr(a, k, t.data_ptr())
    ws = _workspace(dev, need + 16)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    _lib.check(_lib.load().bts_train_vis(C.byref(a), _stream(alphas)), "bts_train_vis")
    return out


# --------------------------------------------------------------------------------------------------------------
# the Monodepth2 decoder's tail: reflect-pad 3x3 convolution [+ nearest x2 in front] [+ ELU], channels-last
# --------------------------------------------------------------------------------------------------------------
def _conv_struct(x, weight, bias, y, N, H, W, up2, elu, out_nchw):
    return _lib.BtsConv3x3(N=N, H=H, W=W, C=x.shape[-1], up2=int(up2), elu=int(elu), out_nchw=int(out_nchw), reserved_=0, x=x.data_ptr(),
                           weight=weight.data_ptr(), bias=_addr(bias), y=_addr(y))


def conv3x3_fwd(x, weight, bias, up2=False, elu=False, out_nchw=False):
    """x (N, Hs, Ws, C) channels-last, weight (C, C, 3, 3), bias (C) | None -> y (N, H, W, C), or (N, C, H, W) with ``out_nchw``; H, W = 2 Hs,
    2 Ws with ``up2`` (bts_conv3x3_fwd: reflection pad 1 + 3 x 3 convolution, the x2 nearest upsampling in front and the ELU behind fused)."""
    _req(x, "x"), _req(weight, "weight", (x.shape[-1], x.shape[-1], 3, 3))
    if bias is not None:
        _req(bias, "bias", (x.shape[-1],))
    N, Hs, Ws, Cc = x.shape
    H, W = (2 * Hs, 2 * Ws) if up2 else (Hs, Ws)
    y = torch.empty((N, Cc, H, W) if out_nchw else (N, H, W, Cc), device=x.device, dtype=torch.float32)
    c = _conv_struct(x, weight, bias, y, N, H, W, up2, elu, out_nchw)
    _lib.check(_lib.load().bts_conv3x3_fwd(C.byref(c), _stream(x)), "bts_conv3x3_fwd")
    return y


def conv3x3_bwd(x, weight, y, g_y, up2=False, elu=False, out_nchw=False, need=(True, True, True)):
    """-> (d_x | None, d_weight | None, d_bias | None) of conv3x3_fwd (bts_conv3x3_bwd); ``y`` = the forward's output (read for elu')."""
    _req(x, "x"), _req(weight, "weight"), _req(g_y, "g_y", tuple(y.shape))
    N, Hs, Ws, Cc = x.shape
    H, W = (2 * Hs, 2 * Ws) if up2 else (Hs, Ws)
    d_x = torch.empty_like(x) if need[0] else None
    d_w = torch.empty_like(weight) if need[1] else None
    d_b = torch.empty(Cc, device=x.device, dtype=torch.float32) if need[2] else None
    c = _conv_struct(x, weight, None, y, N, H, W, up2, elu, out_nchw)
    lib = _lib.load()
    ws_bytes = int(lib.bts_conv3x3_bwd_workspace(C.byref(c)))
    ws = torch.empty(ws_bytes // 4 + 4, device=x.device, dtype=torch.float32)     # (map-sized: goes back to the caching allocator)
    _lib.check(lib.bts_conv3x3_bwd(C.byref(c), _ptr(g_y), _ptr(ws), ws_bytes, _ptr(d_x), _ptr(d_w), _ptr(d_b), _stream(x)), "bts_conv3x3_bwd")
    return d_x, d_w, d_b


class Conv3x3Function(torch.autograd.Function):
    """layers.py:11-40 (Conv3x3 / ConvBlock) [+ the decoder's nearest x2, monodepth2.py:225] as one differentiable op on channels-last
    tensors: (x (N, Hs, Ws, C), weight, bias | None, up2, elu, out_nchw) -> y."""

    @staticmethod
    def forward(ctx, x, weight, bias, up2, elu, out_nchw):
        x, weight = x.contiguous(), weight.contiguous()
        y = conv3x3_fwd(x, weight, None if bias is None else bias.contiguous(), up2, elu, out_nchw)
        ctx.flags = (bool(up2), bool(elu), bool(out_nchw), bias is not None)
        ctx.save_for_backward(x, weight, y if elu else x.new_empty(0))
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        up2, elu, out_nchw, has_bias = ctx.flags
        if not elu:      # (a plain convolution's backward does not read its output: only the shape matters)
            N, Hs, Ws, Cc = x.shape
            H, W = (2 * Hs, 2 * Ws) if up2 else (Hs, Ws)
            y = g
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2])
        d_x, d_w, d_b = conv3x3_bwd(x, weight, y, g.contiguous(), up2, elu, out_nchw, need)
        return d_x, d_w, d_b, None, None, None


def mlp_tensor_sizes(cfg):
    """Element counts of the density MLP's parameter tensors in the packed vector's order (include/bts_render.h): lin_in.weight, lin_in.bias,
    per block fc_0.weight, fc_0.bias, fc_1.weight, fc_1.bias, then lin_out.weight, lin_out.bias."""
    hd, d_in = int(cfg.d_hidden), int(cfg.C) + 3 + 6 * int(cfg.num_freqs)
    return [hd * d_in, hd] + [hd * hd, hd, hd * hd, hd] * int(cfg.n_blocks) + [hd, 1]


def mlp_image_floats(spec) -> int:
    """Floats of bts_eval_frame_prep's ``mlp_image`` scratch for this field (the MLP as the render kernel stages it into LDS)."""
    cfg = _spec_cfg(spec)
    return int(_lib.load().bts_mlp_image_floats(C.byref(cfg)))


def eval_frame(fr, stream, rgb_gt=None):
    """bts_eval_frame on a filled ``_lib.BtsEvalFrame`` (behindthescenes_amd.train_step.FusedEvalFrame builds it).  With ``rgb_gt`` -- a
    contiguous float32 (n, v, 3, H, W) tensor, given here or set as ``fr.rgb_gt`` -- bts_eval_frame_gt: the hand-over launch also writes
    ``images * img_scale + img_shift`` into it.  With ``fr.sched`` -- 256 int32 words on the device, the frame's own while it runs --
    bts_eval_frame_sched: the render's waves claim the last part of the rays from its counters instead of walking fixed lists to the end.
    With ``fr.prep`` -- ``dict(params=[the MLP's tensors], packed=scratch, image=scratch or None)`` -- bts_eval_frame_prep: the projection's
    launch also reads the parameter tensors themselves, packs and stages them (``fr.mlp_params`` is not read), with or without ``sched`` and ``rgb_gt``;
    ``fr.pinned = False``: bts_eval_frame_prep_unpinned, the same frame without the render kernel that has the frame's switches compiled in."""
    if rgb_gt is None:
        rgb_gt = fr.rgb_gt
    sched = getattr(fr, "sched", None)
    prep = getattr(fr, "prep", None)
    if rgb_gt is not None:
        c = fr.cfg
        _req(rgb_gt, "rgb_gt", (c.n, fr.v, 3, c.H, c.W))
    if sched is not None:      # (this and the prep checks run once per FRAME: one inline expression each, not a call per tensor)
        if not sched.is_cuda or sched.dtype != torch.int32 or sched.numel() < 256 or not sched.is_contiguous():
            raise BtsNativeError("sched: 256 contiguous int32 words on the device expected")
    if prep is not None:
        lib = _lib.load()
        sizes = mlp_tensor_sizes(fr.cfg)
        params = list(prep["params"])
        if len(params) != len(sizes) or len(params) > _lib.BTS_MLP_MAX_TENSORS:
            raise BtsNativeError(f"prep: {len(sizes)} parameter tensors expected (lin_in, the blocks, lin_out: weight and bias), got {len(params)}")
        mt = _lib.BtsMlpTensors()
        mt.n_tensors = len(params)
        for i, (t, want) in enumerate(zip(params, sizes)):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != want:
                raise BtsNativeError(f"prep: parameter tensor {i} must be {want} contiguous float32 values on the device (got {tuple(t.shape)}, {t.dtype})")
            mt.tensor[i] = t.data_ptr()
        packed, image = prep["packed"], prep.get("image")
        for name, t, want in (("packed", packed, sum(sizes)), ("image", image, int(lib.bts_mlp_image_floats(C.byref(fr.cfg))))):
            if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < want or want <= 0):
                raise BtsNativeError(f"prep: {name} must be {want} contiguous float32 values on the device")
        entry = lib.bts_eval_frame_prep if getattr(fr, "pinned", True) else lib.bts_eval_frame_prep_unpinned
        _lib.check(entry(C.byref(fr), _ptr(rgb_gt), _ptr(sched), C.byref(mt), _ptr(packed), _ptr(image), stream), "bts_eval_frame_prep")
        return
    if sched is not None:
        _lib.check(_lib.load().bts_eval_frame_sched(C.byref(fr), _ptr(rgb_gt), _ptr(sched), stream), "bts_eval_frame_sched")
        return
    if rgb_gt is None:
        _lib.check(_lib.load().bts_eval_frame(C.byref(fr), stream), "bts_eval_frame")
        return
    _lib.check(_lib.load().bts_eval_frame_gt(C.byref(fr), _ptr(rgb_gt), stream), "bts_eval_frame_gt")


def train_step_fwd(st, stream):
    """bts_train_step_fwd on a filled ``_lib.BtsTrainStep`` (behindthescenes_amd.train_step builds it)."""
    _lib.check(_lib.load().bts_train_step_fwd(C.byref(st), stream), "bts_train_step_fwd")


def train_step_bwd(st, g_loss, stream):
    """bts_train_step_bwd: ``g_loss`` a 0-dim float32 device tensor (the upstream gradient of the loss) or None (= 1)."""
    _lib.check(_lib.load().bts_train_step_bwd(C.byref(st), _ptr(g_loss), stream), "bts_train_step_bwd")


# --------------------------------------------------------------------------------------------------------------
# autograd glue
# --------------------------------------------------------------------------------------------------------------
# The gradient of a projected map G is SPARSE in a training step: the rays of a few thousand 8 x 8 patches reach 8-15 % of its texels,
# yet as a dense autograd tensor it costs a map-sized zero fill, and a full read in the projection's backward (at exp_kitti_360.yaml's
# batch 503 MB each -- as much as everything else the backward moves).  When exactly ONE render reads a map that ProjectFunction made,
# RenderFunction.backward therefore adds into a kept (d_proj, tile flags) pair that is all zero between steps, and
# ProjectFunction.backward reads the flagged tiles only and returns the pair to zero (bts_project_features_bwd_tiles).  Every other
# constellation -- several renders of one map, a hook or retain_grad on G, somebody touching the gradient on its way -- takes the dense
# path; the results are the same either way (tests/test_gpu_sparse_grad.py).
SPARSE_PROJ_GRAD = True


class ProjLink:
    """Ties a map made by ProjectFunction to the RenderFunction calls that read it (FieldTensors.proj_link)."""
    __slots__ = ("renders", "entry", "__weakref__")

    def __init__(self):
        self.renders, self.entry = 0, None


class _SparseGrad:
    __slots__ = ("buf", "tiles", "busy", "version", "owner")


def _reclaim_stale(entry):
    """A busy pair whose map is gone -- the projection's backward never ran for it (torch.autograd.grad(loss, [G]), `inputs=` without the
    encoder, an interrupted backward): the ProjLink it was lent to died with its graph.  The pair is zeroed and free again; without this
    every later step would silently take the dense path and the map-sized buffer would stay pinned half written."""
    if entry.busy and (entry.owner is None or entry.owner() is None or entry.owner().entry is not entry):
        entry.buf.zero_(), entry.tiles.zero_()
        entry.busy = False


_SPARSE = {}


def _sparse_grad(ft: "FieldTensors"):
    g = ft.proj_nhwc
    key = (g.device, tuple(g.shape), torch.cuda.current_stream(g.device).cuda_stream)
    e = _SPARSE.get(key)
    if e is None:
        e = _SparseGrad()
        e.buf = torch.zeros(g.shape, device=g.device, dtype=torch.float32)
        e.tiles = torch.zeros((g.shape[0], proj_tile_count(ft.spec, g.shape[1], g.shape[2])), device=g.device, dtype=torch.uint8)
        e.busy, e.owner = False, None
        _SPARSE[key] = e
    return e


def release_sparse_grads():
    """Drops the kept (d_proj, tile flags) pairs (one map-sized buffer per map shape, device and stream)."""
    _SPARSE.clear()


class ProjectFunction(torch.autograd.Function):
    """(F nchw, packed mlp params) -> G nhwc.  Backward: per-pixel GEMMs in bts_project_features_bwd (_tiles)."""

    @staticmethod
    def forward(ctx, feat_nchw, mlp_params, spec, link=None, tiles=None):
        feat_nchw = as_feature_map(feat_nchw)
        ctx.set_materialize_grads(False)
        ctx.spec, ctx.link = spec, link
        ctx.save_for_backward(feat_nchw, mlp_params)
        return project_features(spec, feat_nchw, mlp_params.contiguous(), tiles)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None
        feat_nchw, mlp_params = ctx.saved_tensors
        need = ctx.needs_input_grad[:2]
        entry = ctx.link.entry if ctx.link is not None else None
        if entry is not None:
            ctx.link.entry = None
            if g.data_ptr() == entry.buf.data_ptr() and entry.buf._version == entry.version and g.shape == entry.buf.shape:
                d_feat, d_mlp = project_features_bwd(ctx.spec, feat_nchw, entry.buf, mlp_params, *need, tiles=entry.tiles, clear_after=True)
                entry.busy = False
                return d_feat, d_mlp, None, None, None
        d_feat, d_mlp = project_features_bwd(ctx.spec, feat_nchw, g.contiguous(), mlp_params, *need)
        if entry is not None:   # the kept pair was replaced or modified on its way here: dense on what arrived, and the pair starts over
            entry.buf.zero_(), entry.tiles.zero_()
            entry.busy = False
        return d_feat, d_mlp, None, None, None


def _prep_grad(g, present=True):
    """An upstream gradient as the backward takes it: contiguous, or None where there is none (or its output was not requested)."""
    return g.contiguous() if (g is not None and present and g.numel() > 0) else None


def _empty_feature_chain(spec, mlp_params, empty_feature, d_eproj, d_mlp, need_empty, need_mlp):
    """The projected empty feature is w_in[:, :C] @ empty_feature (a 64x64 GEMV): the chain rule on parameter-sized tensors.  Adds the
    weights' part into d_mlp and returns d_empty_feature (or None)."""
    if d_eproj is None:
        return None
    w_f = mlp_params[:spec.d_hidden * spec.d_in].view(spec.d_hidden, spec.d_in)[:, :spec.C]
    if need_mlp:
        d_mlp[:spec.d_hidden * spec.d_in].view(spec.d_hidden, spec.d_in)[:, :spec.C] += torch.outer(d_eproj, empty_feature.detach())
    return w_f.t() @ d_eproj if need_empty else None


class RenderFunction(torch.autograd.Function):
    """composite() as one differentiable op.  Differentiable inputs: proj_nhwc (G), mlp_params, empty_feature.
    Differentiable outputs: rgb, depth, weights, alphas (invalid / rgb_samps carry no gradient, as in the reference where
    they only depend on poses and colours)."""

    @staticmethod
    def forward(ctx, proj_nhwc, mlp_params, empty_feature, ft: FieldTensors, rays, z_samp, hard_alpha_cap, white_bkgd,
                want_weights, want_alphas, want_rgb_samps, grad_mode=True, want_invalid=True, want_invalid_sums=False, sigma_noise=None,
                jitter=None, lindisp=True, want_z=False):
        # needs_input_grad reflects requires_grad even under torch.no_grad(), and inside forward() grad mode is always off: the
        # caller passes the mode it was invoked in, so that evaluation does not allocate / write the 8 B per sample of saved state
        # (outputs nobody differentiates through arrive as None in backward, not as zero-filled tensors of their size: in a lean training
        # step that was four fills per render -- rgb_samps, z_samp, the two per-ray reductions)
        ctx.set_materialize_grads(False)
        needs_grad = any(ctx.needs_input_grad[:3]) and grad_mode
        # z_samp None: sample_coarse inside the kernel from `jitter`; the depths are materialised only for the backward / on request
        out = render_fwd(ft, mlp_params, rays, z_samp, hard_alpha_cap=hard_alpha_cap, white_bkgd=white_bkgd,
                         want_weights=want_weights, want_alphas=want_alphas, want_invalid=want_invalid, want_rgb_samps=want_rgb_samps,
                         want_saved=needs_grad, want_invalid_sums=want_invalid_sums, sigma_noise=sigma_noise, jitter=jitter, lindisp=lindisp,
                         want_z=want_z or needs_grad)
        ctx.ft, ctx.hard_alpha_cap, ctx.white_bkgd = ft, hard_alpha_cap, white_bkgd
        ctx.link = getattr(ft, "proj_link", None) if (needs_grad and ctx.needs_input_grad[0]) else None
        if ctx.link is not None:
            ctx.link.renders += 1
        ctx.sigma_noise = sigma_noise if needs_grad else None      # (a plain tensor without graph: kept on the context)
        if needs_grad:
            # rgb_samps is non-differentiable output the caller asked for: kept for the backward too (it then skips the colour taps)
            ctx.save_for_backward(mlp_params, rays, out["z_samp"], out["sigma_raw"], out["trans"], *([out["rgb_samps"]] if want_rgb_samps else []))
        empty = rays.new_empty(0)
        z_out = out["z_samp"] if (z_samp is None and out["z_samp"] is not None) else empty
        res = (out["rgb"], out["depth"], out["weights"] if want_weights else empty, out["alphas"] if want_alphas else empty,
               out["invalid"] if want_invalid else empty, out["rgb_samps"] if want_rgb_samps else empty,
               out["invalid_wsum"] if want_invalid_sums else empty, out["invalid_any"] if want_invalid_sums else empty, z_out)
        ctx.mark_non_differentiable(*res[4:])
        ctx.has = (want_weights, want_alphas)
        return res

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_weights, g_alphas, _g_inv, _g_rs, _g_iw, _g_ia, _g_z):
        mlp_params, rays, z_samp, sigma_raw, trans, *rest = ctx.saved_tensors
        rgb_samps = rest[0] if rest else None
        prep, ft = _prep_grad, ctx.ft
        need_proj, need_mlp, need_empty = ctx.needs_input_grad[:3]
        pg, link, G, entry = None, ctx.link, ft.proj_nhwc, None
        if (need_proj and SPARSE_PROJ_GRAD and link is not None and link.renders == 1 and link.entry is None and not G.retains_grad
                and not G._backward_hooks):
            entry = _sparse_grad(ft)
            _reclaim_stale(entry)
            if not entry.busy:
                entry.busy, entry.version, link.entry = True, entry.buf._version, entry
                entry.owner = weakref.ref(link)
                pg = (entry.buf, entry.tiles)
            else:
                entry = None
        try:
            d_proj, d_mlp, d_eproj = render_bwd(ft, mlp_params, rays, z_samp, sigma_raw, trans, hard_alpha_cap=ctx.hard_alpha_cap,
                                                g_rgb=prep(g_rgb), g_depth=prep(g_depth), g_weights=prep(g_weights, ctx.has[0]), white_bkgd=ctx.white_bkgd,
                                                rgb_samps=rgb_samps, g_alphas=prep(g_alphas, ctx.has[1]), need_proj=need_proj, need_mlp=need_mlp,
                                                need_empty=need_empty or (need_mlp and ft.spec.learn_empty), sigma_noise=ctx.sigma_noise, proj_grad=pg)
        except Exception:
            if pg is not None:      # a failed launch may have left the kept pair half written: it starts over, and the link forgets it
                entry.buf.zero_(), entry.tiles.zero_()
                entry.busy, link.entry = False, None
            raise
        d_empty = _empty_feature_chain(ft.spec, mlp_params, ft.empty_feature, d_eproj, d_mlp, need_empty, need_mlp)
        return (d_proj, d_mlp, d_empty) + (None,) * 15


class MultiViewRenderFunction(torch.autograd.Function):
    """composite() over merged encoder views (MultiViewField) as one differentiable op.  Differentiable inputs: mlp_params, empty_feature
    and every view's projected map (the trailing arguments); differentiable outputs: rgb, depth, weights, alphas."""

    @staticmethod
    def forward(ctx, mlp_params, empty_feature, ft: MultiViewField, rays, z_samp, hard_alpha_cap, white_bkgd, want_weights, want_alphas,
                want_rgb_samps, grad_mode, want_invalid, sigma_noise, jitter, lindisp, want_z, *projs):
        ctx.set_materialize_grads(False)
        needs_grad = any(ctx.needs_input_grad[:2] + ctx.needs_input_grad[16:]) and grad_mode
        # rgb_samps is kept for the backward as well (it then skips the colour taps)
        out = render_fwd(ft, mlp_params, rays, z_samp, hard_alpha_cap=hard_alpha_cap, white_bkgd=white_bkgd, want_weights=want_weights,
                         want_alphas=want_alphas, want_invalid=want_invalid, want_rgb_samps=want_rgb_samps or needs_grad, want_saved=needs_grad,
                         sigma_noise=sigma_noise, jitter=jitter, lindisp=lindisp, want_z=want_z or needs_grad)
        ctx.ft, ctx.hard_alpha_cap, ctx.white_bkgd = ft, hard_alpha_cap, white_bkgd
        ctx.sigma_noise = sigma_noise if needs_grad else None
        if needs_grad:
            ctx.save_for_backward(mlp_params, rays, out["z_samp"], out["sigma_raw"], out["trans"], out["rgb_samps"])
        empty = rays.new_empty(0)
        z_out = out["z_samp"] if (z_samp is None and out["z_samp"] is not None) else empty
        res = (out["rgb"], out["depth"], out["weights"] if want_weights else empty, out["alphas"] if want_alphas else empty,
               out["invalid"] if want_invalid else empty, out["rgb_samps"] if want_rgb_samps else empty, z_out)
        ctx.mark_non_differentiable(*res[4:])
        ctx.has = (want_weights, want_alphas)
        return res

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_weights, g_alphas, _g_inv, _g_rs, _g_z):
        mlp_params, rays, z_samp, sigma_raw, trans, rgb_samps = ctx.saved_tensors
        prep, ft = _prep_grad, ctx.ft
        need_mlp, need_empty = ctx.needs_input_grad[:2]
        d_projs, d_mlp, d_eproj = render_bwd_multi_view(
            ft, mlp_params, rays, z_samp, sigma_raw, trans, hard_alpha_cap=ctx.hard_alpha_cap, g_rgb=prep(g_rgb), g_depth=prep(g_depth),
            g_weights=prep(g_weights, ctx.has[0]), g_alphas=prep(g_alphas, ctx.has[1]), need_proj=ctx.needs_input_grad[16:], need_mlp=need_mlp,
            need_empty=need_empty or (need_mlp and ft.spec.learn_empty), white_bkgd=ctx.white_bkgd, rgb_samps=rgb_samps, sigma_noise=ctx.sigma_noise)
        d_empty = _empty_feature_chain(ft.spec, mlp_params, ft.empty_feature, d_eproj, d_mlp, need_empty, need_mlp)
        return (d_mlp, d_empty) + (None,) * 14 + tuple(d_projs)
