"""The two functions every demo script of the reference funnels through -- ``render_poses`` (scripts/inference_setup.py:182-198) and
``color_tensor`` (utils/plotting.py:41-46) -- and the per-frame lines around them (scripts/videos/gen_vid_nvs.py:102-120,
gen_vid_transition.py:111-171, gen_vid_seq.py:108-137) on the HIP kernels of csrc/bts_frames.hip.

``color_tensor`` and ``render_poses`` keep the reference's signatures and results, so the scripts bind with

    from behindthescenes_amd.novel_views import color_tensor, render_poses

``FusedNovelViews`` runs a whole trajectory from a field that is encoded once: per chunk of poses ONE library call
(``bts_novel_views``: rays, the render with ``sample_coarse`` inside and the epilogue's ``invalid_wsum``, the frame maximum, the finish
kernel) that ends in uint8 panels of a ``(P, Hc, Wc, 3)`` canvas on the device; the caller's single ``.cpu()`` is the only copy of a
trajectory.  ``colorize_u8`` / ``pack_u8`` put further panels (the occupancy profile, the input image) into the same canvas.
The colour map is matplotlib's own table (``Colormap._lut``), looked up once per name and device; matplotlib is imported only when a
name has to be resolved.  There is no torch fallback: CPU tensors are rejected, as everywhere else in this package."""
import numpy as np
import torch

from . import _lib, native
from ._lib import BtsNativeError

LAYOUTS = ("image_over_depth", "image", "depth")
_HOST_TABLES = {}     # name -> (N, (N + 3, 3) float64, (N + 3, 3) uint8)
_DEVICE_TABLES = {}   # (name, device) -> (N, float64 tensor, uint8 tensor)


def cmap_table(cmap):
    """``cmap``: a matplotlib colour-map name, or the table itself as matplotlib holds it -- an ``(N + 3, 3 | 4)`` array whose rows N,
    N + 1, N + 2 are the under, over and bad colours.  Returns (N, lut (N + 3, 3) float64, (lut * 255).astype(uint8)) on the host."""
    if isinstance(cmap, str):
        hit = _HOST_TABLES.get(cmap)
        if hit is not None:
            return hit
        try:
            import matplotlib
        except ImportError as e:
            raise BtsNativeError(f"colour map {cmap!r}: resolving a name needs matplotlib; pass the (N + 3, 3) table instead") from e
        try:
            cm = matplotlib.colormaps[cmap] if hasattr(matplotlib, "colormaps") else matplotlib.cm.get_cmap(cmap)
        except (KeyError, ValueError) as e:
            raise BtsNativeError(f"colour map {cmap!r} is not known to matplotlib") from e
        cm._init()
        lut = np.asarray(cm._lut, dtype=np.float64)
    else:
        if isinstance(cmap, torch.Tensor):
            cmap = cmap.detach().cpu().numpy()
        lut = np.asarray(cmap, dtype=np.float64)
    if lut.ndim != 2 or lut.shape[1] not in (3, 4) or lut.shape[0] < 4 or lut.shape[0] - 3 > _lib.BTS_CMAP_MAX_N:
        raise BtsNativeError(f"colour map: an (N + 3, 3 | 4) table with 1 <= N <= {_lib.BTS_CMAP_MAX_N} expected, got {lut.shape}")
    lut = np.ascontiguousarray(lut[:, :3])
    out = (lut.shape[0] - 3, lut, (lut * 255).astype(np.uint8))
    if isinstance(cmap, str):
        _HOST_TABLES[cmap] = out
    return out


def _device_table(cmap, device):
    key = (cmap, device) if isinstance(cmap, str) else None
    if key is not None and key in _DEVICE_TABLES:
        return _DEVICE_TABLES[key]
    N, lut, lut_u8 = cmap_table(cmap)
    out = (N, torch.from_numpy(lut).to(device), torch.from_numpy(lut_u8).to(device))
    if key is not None:
        _DEVICE_TABLES[key] = out
    return out


def _gpu_f32(t, name):
    if not isinstance(t, torch.Tensor):
        raise BtsNativeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise BtsNativeError(f"{name}: must live on the GPU (got {t.device}); the HIP renderer has no CPU path")
    if t.dtype != torch.float32:
        raise BtsNativeError(f"{name}: must be float32 (got {t.dtype})")
    return t


def color_tensor(tensor, cmap, norm=False):
    """utils/plotting.py:41-46: ``tensor (...)`` float32 -> ``(..., 3)`` float64 colours on the tensor's device, with no host copy.
    ``norm``: (tensor - tensor.min()) / (tensor.max() - tensor.min()) over the WHOLE tensor first, as there."""
    _gpu_f32(tensor, "tensor")
    if tensor.numel() == 0:
        return torch.empty(tuple(tensor.shape) + (3,), device=tensor.device, dtype=torch.float64)
    N, lut, _ = _device_table(cmap, tensor.device)
    out = native.colorize(tensor.contiguous().view(1, 1, -1), N, lut_f64=lut, norm=norm)
    return out.view(tuple(tensor.shape) + (3,))


def colorize_u8(x, cmap, norm, canvas, row0=0, col0=0):
    """``x (B, h, w)`` or ``(h, w)`` float32 -> the colour map's bytes into ``canvas (B, Hc, Wc, 3)`` at (row0, col0); ``norm`` per image.
    (The occupancy profile's panel: gen_vid_seq.py:126-131.)"""
    _gpu_f32(x, "x")
    if x.dim() == 2:
        x = x.unsqueeze(0)
    N, _, lut_u8 = _device_table(cmap, x.device)
    native.colorize(x.contiguous(), N, lut_u8=lut_u8, norm=norm, want_f64=False, canvas=canvas, row0=row0, col0=col0)
    return canvas


def pack_u8(x, canvas, row0=0, col0=0, scale=1.0, shift=0.0, channels_first=False):
    """A float image as bytes of ``x * scale + shift`` into ``canvas`` at (row0, col0): ``x (B, h, w, 3)``, or ``(B, 3, h, w)`` with
    ``channels_first`` (the input-image panel: ``images * .5 + .5``).  Read where it lies, through its strides."""
    _gpu_f32(x, "x")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if channels_first:
        x = x.permute(0, 2, 3, 1)
    return native.pack_u8(x, canvas, row0, col0, scale, shift)


def _why_not(wrapped, sampler):
    from .ray_sampler import ImageRaySampler
    from .renderer import NeRFRenderer
    net, r = getattr(wrapped, "net", None), getattr(wrapped, "renderer", None)
    if not isinstance(r, NeRFRenderer) or not isinstance(sampler, ImageRaySampler) or getattr(wrapped, "simple_output", False) or net is None:
        return "needs behindthescenes_amd's NeRFRenderer (bind_parallel, simple_output=False) and ImageRaySampler"
    if r.using_fine or r.n_fine:
        return "a fine pass (n_fine > 0)"
    if r.sched is not None:
        return "a sampling schedule"
    if r.white_bkgd:
        return "a white background"
    if r.training and r.noise_std > 0.0:
        return "density noise in training mode"
    if getattr(r.sample_coarse, "__func__", None) is not NeRFRenderer.sample_coarse:
        return "sample_coarse is overridden"
    if not net.sample_color:
        return "sample_color=False (MLP-predicted colours: the novel-view call serves sampled colours only)"
    if net.torch_mode:
        return "a PyTorch-composed field mode (merged encoder views)"
    if getattr(net, "multi_view", False):
        return "more than one encoder view (native_multi_view renders entry by entry)"
    if getattr(net, "_patch", 0) or sampler.channels == 27:
        return native.PATCH_COLOR_MESSAGE
    if sampler.channels != 3 or sampler.height is None or sampler.width is None:
        return "the sampler needs height, width and three channels"
    src = getattr(net, "_grid_c_src", None)
    if not getattr(net, "_has_latents", False) or src is None:
        return "no field state: call net.encode(images, projs, poses, ids_encoder=[0], ids_render=[0]) first"
    if src.shape[0] != 1 or src.shape[1] != 1:
        return f"n = {src.shape[0]}, nv = {src.shape[1]}: the scripts render from one encoded sample with one colour view (ids_render=[0])"
    return None


def _pinned_to(rows, device):
    t = torch.tensor(rows, dtype=torch.float32)
    return t.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else t.to(device)


def _per_pose(x, P, name):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().tolist()
    if isinstance(x, (int, float)):
        return [float(x)] * P
    x = [float(v) for v in x]
    if len(x) != P:
        raise BtsNativeError(f"{name}: a number or one per pose ({P}) expected, got {len(x)}")
    return x


class FusedNovelViews:
    """A trajectory of novel views of ONE encoded field as uint8 frames on the device.

        net.encode(images, projs, poses, ids_encoder=[0], ids_render=[0]); net.set_scale(0)
        nv = FusedNovelViews(wrapped, ImageRaySampler(z_near, z_far, h, w, norm_dir=False), cmap="magma")
        frames = nv.frames(poses_nv, projs[0, 0], d_min, d_max).cpu().numpy()       # (P, 2 h, w, 3) uint8, image over depth

    ``frames`` runs chunks of ``poses_per_call`` poses, one ``bts_novel_views`` call each, and synchronises nothing.  ``layout``:
    "image_over_depth" (gen_vid_nvs.py:110), "image" or "depth"; with ``canvas`` (a zero-filled ``(P, Hc, Wc, 3)`` uint8 tensor of the
    caller) ``offsets = ((image_row0, image_col0) | None, (depth_row0, depth_col0) | None)`` places the panels (gen_vid_seq's profile
    to the right, gen_vid_transition's centred narrower frames: one call per width).  ``d_min`` / ``d_max``: the depth panel's range,
    numbers or one per pose; ``near_far``: ``(P, 2)`` ray ranges, default the sampler's.  ``jitter (P * h * w, K)`` replaces the
    ``torch.rand`` draw of every chunk (the deterministic seam, as on ``FusedEvalFrame``)."""

    def __init__(self, wrapped, sampler, cmap="magma", poses_per_call=8):
        if int(poses_per_call) <= 0:
            raise BtsNativeError(f"poses_per_call: a positive number expected, got {poses_per_call}")
        self.wrapped, self.sampler, self.cmap, self.poses_per_call = wrapped, sampler, cmap, int(poses_per_call)
        cmap_table(cmap)              # an unknown name fails here, not in the middle of a trajectory
        self._scratch = {}

    def why_not(self):
        return _why_not(self.wrapped, self.sampler)

    def _buffers(self, dev, P, h, w):
        key = (dev, P, h, w)
        sc = self._scratch.get(key)
        if sc is None:
            f32 = dict(device=dev, dtype=torch.float32)
            sc = self._scratch[key] = dict(rays=torch.empty((P * h * w, 8), **f32), wsum=torch.empty((P * h * w,), **f32),
                                           fmax=torch.empty((P, _lib.BTS_FRAMES_PARTIALS, 3), **f32),
                                           rgb=torch.empty((P, h, w, 3), **f32), depth=torch.empty((P, h, w), **f32))
        return sc

    @torch.no_grad()
    def render(self, poses, projs, near_far=None, norm_range=None, black_invalid=False, canvas=None, offsets=(None, None), jitter=None,
               rgb=None, depth=None):
        """The chunked calls on validated device tensors: poses (P, 4, 4), projs (P, 3, 3), near_far (P, 2), norm_range (P, 2) or None.
        Writes into ``canvas`` and, when given, the masked floats into ``rgb (P, h, w, 3)`` / ``depth (P, h, w)``."""
        reason = self.why_not()
        if reason is not None:
            raise BtsNativeError("FusedNovelViews: " + reason)
        net, r, smp = self.wrapped.net, self.wrapped.renderer, self.sampler
        h, w, K, P = int(smp.height), int(smp.width), int(r.n_coarse), int(poses.shape[0])
        dev = poses.device
        ft = net.native_field()
        params = net.mlp_coarse.packed().detach()
        if jitter is not None:
            native._req(jitter, "jitter", (P * h * w, K))
        N, lut_u8 = 0, None
        (img_off, dep_off) = offsets
        if canvas is not None and dep_off is not None:
            N, _, lut_u8 = _device_table(self.cmap, dev)
            if norm_range is None:
                raise BtsNativeError("the depth panel needs d_min / d_max")
        stream = native._stream(poses)
        for c0 in range(0, P, self.poses_per_call):
            c1 = min(P, c0 + self.poses_per_call)
            Pc = c1 - c0
            sc = self._buffers(dev, Pc, h, w)
            u = jitter[c0 * h * w:c1 * h * w] if jitter is not None else torch.rand((Pc * h * w, K), device=dev, dtype=torch.float32)
            o_rgb = rgb[c0:c1] if rgb is not None else sc["rgb"]
            o_depth = depth[c0:c1] if depth is not None else sc["depth"]
            a = _lib.BtsNovelViews(P=Pc, h=h, w=w, K=K, lindisp=int(bool(r.lindisp)), hard_alpha_cap=int(bool(r.hard_alpha_cap)),
                                   norm_dir=int(bool(smp.norm_dir)), black_invalid=int(bool(black_invalid)),
                                   write_masked=int(rgb is not None or depth is not None), finish_only=0, lut_N=N, reserved_=0,
                                   poses_c2w=poses[c0:c1].data_ptr(), Ks=projs[c0:c1].data_ptr(), near_far=near_far[c0:c1].data_ptr(),
                                   norm_range=None if norm_range is None else norm_range[c0:c1].data_ptr(), jitter=u.data_ptr(),
                                   rays=sc["rays"].data_ptr(), invalid_wsum=sc["wsum"].data_ptr(), frame_max=sc["fmax"].data_ptr(),
                                   rgb=o_rgb.data_ptr(), depth=o_depth.data_ptr(), lut_u8=None if lut_u8 is None else lut_u8.data_ptr(),
                                   canvas=None if canvas is None else canvas[c0:c1].data_ptr(),
                                   Hc=0 if canvas is None else int(canvas.shape[1]), Wc=0 if canvas is None else int(canvas.shape[2]),
                                   img_row0=-1 if img_off is None else int(img_off[0]), img_col0=0 if img_off is None else int(img_off[1]),
                                   depth_row0=-1 if dep_off is None else int(dep_off[0]), depth_col0=0 if dep_off is None else int(dep_off[1]))
            native.novel_views(ft, params, a, stream)
        return canvas

    def _cameras(self, poses, projs, near_far):
        smp = self.sampler
        if not isinstance(poses, torch.Tensor) or not poses.is_cuda:
            raise BtsNativeError("poses: a (P, 4, 4) tensor on the GPU expected; the HIP renderer has no CPU path")
        poses = poses.detach().float().reshape(-1, 4, 4).contiguous()
        P, dev = poses.shape[0], poses.device
        if P == 0:
            raise BtsNativeError("poses: an empty trajectory")
        if not isinstance(projs, torch.Tensor) or projs.numel() not in (9, 9 * P):
            raise BtsNativeError(f"projs: one (3, 3) matrix or one per pose ({P}) expected")
        projs = projs.detach().float().to(dev).reshape(-1, 3, 3).expand(P, 3, 3).contiguous()
        if near_far is None:
            nf = [[float(smp.z_near), float(smp.z_far)]] * P
        else:
            nf = near_far.detach().cpu().tolist() if isinstance(near_far, torch.Tensor) else [[float(a), float(b)] for a, b in near_far]
            if len(nf) != P:
                raise BtsNativeError(f"near_far: (P, 2) = ({P}, 2) expected")
        return poses, projs, nf

    def frames(self, poses, projs, d_min, d_max, near_far=None, black_invalid=False, layout="image_over_depth", canvas=None, offsets=None,
               jitter=None):
        """-> ``(P, Hc, Wc, 3)`` uint8 on the device."""
        if layout not in LAYOUTS:
            raise BtsNativeError(f"layout: one of {LAYOUTS} expected, got {layout!r}")
        reason = self.why_not()
        if reason is not None:
            raise BtsNativeError("FusedNovelViews: " + reason)
        poses, projs, nf = self._cameras(poses, projs, near_far)
        P, dev, h, w = poses.shape[0], poses.device, int(self.sampler.height), int(self.sampler.width)
        if canvas is None:
            if offsets is not None:
                raise BtsNativeError("offsets place the panels in the caller's canvas: pass canvas= too")
            canvas = torch.zeros((P, 2 * h if layout == "image_over_depth" else h, w, 3), device=dev, dtype=torch.uint8)
            offsets = {"image_over_depth": ((0, 0), (h, 0)), "image": ((0, 0), None), "depth": (None, (0, 0))}[layout]
        else:
            if offsets is None or len(offsets) != 2:
                raise BtsNativeError("canvas: offsets=((image_row0, image_col0) | None, (depth_row0, depth_col0) | None) expected with it")
            for off, what in zip(offsets, ("image", "depth")):
                if off is not None:
                    native._req_canvas(canvas, P, h, w, int(off[0]), int(off[1]), what)
        # 1 / d_max and the denominator as the scripts' Python evaluates them, in double, rounded once to fp32 (gen_vid_nvs.py:106)
        lo, hi = _per_pose(d_min, P, "d_min"), _per_pose(d_max, P, "d_max")
        rows = [a + [1 / m, 1 / l - 1 / m] for a, l, m in zip(nf, lo, hi)]
        cam = _pinned_to(rows, dev)                       # ONE small host-to-device copy per trajectory
        near_far_d, norm_range = cam[:, :2].contiguous(), cam[:, 2:].contiguous()
        return self.render(poses, projs, near_far_d, norm_range, black_invalid, canvas, tuple(offsets), jitter)


def finish_views(rgb, depth, invalid_wsum, d_min, d_max, cmap="magma", black_invalid=False, canvas=None, offsets=None):
    """The finish kernel alone, on a render the caller already holds (``bts_novel_views`` with ``finish_only``): ``rgb (P, h, w, 3)``,
    ``depth (P, h, w)`` and ``invalid_wsum (P, h, w)`` = sum_k invalid * weights, contiguous float32.  With ``black_invalid`` the masked
    values are written back IN PLACE (render_poses' return values).  Panels go to ``canvas`` at ``offsets`` as in
    ``FusedNovelViews.frames``; without a canvas a fresh image-over-depth one is returned."""
    P, h, w = (int(v) for v in depth.shape)
    native._req(rgb, "rgb", (P, h, w, 3)), native._req(depth, "depth", (P, h, w)), native._req(invalid_wsum, "invalid_wsum", (P, h, w))
    dev = depth.device
    if canvas is None:
        canvas = torch.zeros((P, 2 * h, w, 3), device=dev, dtype=torch.uint8)
        offsets = ((0, 0), (h, 0))
    img_off, dep_off = offsets
    for off, what in ((img_off, "image"), (dep_off, "depth")):
        if off is not None:
            native._req_canvas(canvas, P, h, w, int(off[0]), int(off[1]), what)
    N, _, lut_u8 = _device_table(cmap, dev)
    lo, hi = _per_pose(d_min, P, "d_min"), _per_pose(d_max, P, "d_max")
    norm_range = _pinned_to([[1 / m, 1 / l - 1 / m] for l, m in zip(lo, hi)], dev)
    fmax = torch.empty((P, _lib.BTS_FRAMES_PARTIALS, 3), device=dev, dtype=torch.float32)
    a = _lib.BtsNovelViews(P=P, h=h, w=w, K=0, black_invalid=int(bool(black_invalid)), write_masked=1, finish_only=1, lut_N=N,
                           norm_range=norm_range.data_ptr(), invalid_wsum=invalid_wsum.data_ptr(), frame_max=fmax.data_ptr(),
                           rgb=rgb.data_ptr(), depth=depth.data_ptr(), lut_u8=lut_u8.data_ptr(), canvas=canvas.data_ptr(),
                           Hc=int(canvas.shape[1]), Wc=int(canvas.shape[2]),
                           img_row0=-1 if img_off is None else int(img_off[0]), img_col0=0 if img_off is None else int(img_off[1]),
                           depth_row0=-1 if dep_off is None else int(dep_off[0]), depth_col0=0 if dep_off is None else int(dep_off[1]))
    native.novel_views(None, None, a, native._stream(depth))
    return canvas


def render_poses(renderer, ray_sampler, poses, projs, black_invalid=False):
    """scripts/inference_setup.py:182-198 with its signature and shapes: ``renderer`` the bound render wrapper, ``poses (1, v, 4, 4)``
    and ``projs (1, v, 3, 3)`` of which view 0 is rendered -> ``frame (1, h, w, 1, 3)``, ``depth (h, w)``, device tensors (the scripts'
    ``.cpu()`` still works).  One ``bts_novel_views`` call with P = 1; the jitter is the renderer's one ``torch.rand`` draw."""
    nv = FusedNovelViews(renderer, ray_sampler, cmap=_NO_CMAP, poses_per_call=1)
    reason = nv.why_not()
    if reason is not None:
        raise BtsNativeError("render_poses: " + reason)
    if not isinstance(poses, torch.Tensor) or poses.dim() != 4 or not isinstance(projs, torch.Tensor) or projs.dim() != 4:
        raise BtsNativeError("render_poses: poses (1, v, 4, 4) and projs (1, v, 3, 3) expected")
    pose, proj, nf = nv._cameras(poses[:1, :1], projs[:1, :1], None)
    h, w, dev = int(ray_sampler.height), int(ray_sampler.width), pose.device
    frame = torch.empty((1, h, w, 3), device=dev, dtype=torch.float32)
    depth = torch.empty((1, h, w), device=dev, dtype=torch.float32)
    nv.render(pose, proj, _pinned_to(nf, dev), None, black_invalid, None, (None, None), None, frame, depth)
    return frame.view(1, h, w, 1, 3), depth[0]


_NO_CMAP = np.zeros((4, 3))     # render_poses writes no colour-mapped panel: a one-entry table nobody reads
