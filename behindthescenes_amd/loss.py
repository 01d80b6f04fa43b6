"""Drop-in for the reference's ``ReconstructionLoss`` (models/bts/model/loss.py:43-293) on the renderer's patch outputs.

For the criterion every shipped config trains with ("l1+ssim") the whole photometric term -- SSIM + L1 per patch, minimum over the
render views, invalid-ray masking, edge-aware smoothness -- and its gradient with respect to ``rgb`` / ``depth`` come from ONE HIP
pass per scale (``bts_photometric_loss``, csrc/bts_loss.hip); the ~60 small kernels and nine ``.item()`` synchronisations of the
reference become one launch, one reduction and one device-to-host copy for the logging dict.  The patch may have any size: up to 64
pixels (every shipped config: ``patch_size: 8``) one wave takes one patch; above that -- the trainer's default ``patch_size = 16``,
``sample_mode: image``, and the validation loss, where ``ImageRaySampler.reconstruct`` hands over whole frames as ``(n, v, H, W, nv, 3)``
-- the patch is cut into 16 x 16 tiles (``bts_photometric_loss_tiled``, csrc/bts_loss_tiled.hip: four launches, under ``no_grad``
three); ``native.photometric_loss`` chooses.  With the config key ``native_pixel_loss: true`` the reference's other options run on
HIP kernels too: criterion "l1" / "l2" with or without ``median_thresholding`` under any invalid policy (``bts_pixel_loss``,
csrc/bts_loss_pixel.hip: ``native.pixel_loss``), and "l1+ssim" under ``weight_guided_diverse`` (``bts_loss_diverse_flags``, then the
kernels above under the strict policy).  With ``native_ssim_median: true`` "l1+ssim" with ``median_thresholding`` runs on the median
variant of the tiled passes (``bts_photometric_loss_median``, csrc/bts_loss_tiled.hip: ``native.photometric_loss_median``; every patch
size, per scale and batch sample its own threshold, the rgb term normalised by the kept count on the device).  With ``native_automask: true``
``use_automasking=True`` runs on the same kernels' ``_automask`` entry points: ``rgb_gt`` then carries the error map of
``automask.automask_images`` as a fourth channel, which bounds every pixel's error (``min(e, thresh)`` after the minimum over the views,
before the invalid-ray mask and the median ranking; torch's binary-min gradient, a tie taking half).  The reference renders that fourth
channel as well and cuts it off first thing; its gradient is exactly 0, so the render kernels keep their three channels and the rendered
``rgb`` arrives with 3.  The optional regularisers (depth /
alpha / surfaceness / depth-smoothness / ray-entropy, all off in the shipped configs) are a few elementwise torch expressions on
top; with ``native_regularisers: true`` every one of them whose lambda is > 0 comes, forward and gradient, from one call per scale
(``bts_loss_regularisers``, csrc/bts_loss_reg.hip: ``native.loss_regularisers``).  Same constructor keys, same call signature, same ``(loss, loss_dict)`` result as the reference."""
import math
from collections.abc import MutableMapping

import torch
from torch.autograd import profiler

from . import native


class _NativeTerms(torch.autograd.Function):
    """One native loss call as an autograd node: ``fn(x, y, need_grad, kw) -> (terms, g_x | None, g_y | None)`` with g_x = d terms[ix] /
    d x and g_y = d terms[iy] / d y written for an upstream gradient of 1; differentiable w.r.t. x and y, each scaled in backward by its
    entry of the upstream gradient.  (x, y) = (rgb, depth) with entries (0, 1) for the photometric terms, (alphas, depth) THROUGH ENTRY 5
    for the regularisers (their terms are read for the logging dict)."""

    @staticmethod
    def forward(ctx, fn, entries, x, y, kw):
        ctx.set_materialize_grads(False)
        terms, g_x, g_y = fn(x, y, ctx.needs_input_grad[2] or ctx.needs_input_grad[3], kw)
        ctx.save_for_backward(g_x, g_y)
        ctx.entries = entries
        return terms

    @staticmethod
    def backward(ctx, g):
        g_x, g_y = ctx.saved_tensors
        if g is None:
            return (None,) * 5
        ix, iy = ctx.entries
        d_x = g_x * g[ix] if (g_x is not None and ctx.needs_input_grad[2]) else None
        d_y = g_y * g[iy] if (g_y is not None and ctx.needs_input_grad[3]) else None
        return None, None, d_x, d_y, None


# the native entries as _NativeTerms' fn (kw: the entry's keywords).  The photometric ones -> (rgb term, sum of the smoothness term, number of invalid rays):
def _photometric_sums(rgb, depth, need_grad, kw):
    """l1+ssim: the three as SUMS over all patches"""
    parts, g_rgb, g_depth = native.photometric_loss(rgb, depth, scale_rgb=1.0, scale_eas=1.0, need_grad=need_grad, **kw)
    return parts.sum(0)[:3], g_rgb, g_depth


def _median_terms(rgb, depth, need_grad, kw):
    """l1+ssim with median thresholding: the rgb term arrives normalised by the kept count"""
    out, _, _, g_rgb, g_depth = native.photometric_loss_median(rgb, depth, need_grad=need_grad, **kw)
    return out[:3], g_rgb, g_depth


def _pixel_terms(rgb, depth, need_grad, kw):
    """l1 / l2: the rgb term arrives normalised -- by 3 B, or with median thresholding by the kept count"""
    out, _, _, g_rgb, g_depth = native.pixel_loss(rgb, depth, need_grad=need_grad, **kw)
    return out[:3], g_rgb, g_depth


def _pixel_c_terms(rgb, depth, need_grad, kw):
    """l1 / l2 on other than 3 colour channels: the rgb term arrives normalised by C B; no smoothness term"""
    out, g_rgb = native.pixel_loss_channels(rgb, need_grad=need_grad, **kw)
    return out[:3], g_rgb, None


def _reg_terms(alphas, depth, need_grad, kw):
    """one scale's regularisers as one (6,) tensor: [alpha_reg, surfaceness, entropy, depth term, invalid rays, reg = sum_t coef_t term_t]"""
    _, _, g_alphas, g_depth, out = native.loss_regularisers_packed(alphas, depth, need_grad=need_grad, **kw)
    return out, g_alphas, g_depth


_MASKS = ("weights", "invalid", "invalid_wsum", "invalid_any", "rgb_samps")      # the invalid-ray inputs, by the native entries' keywords


def _flat(t, tail):
    """(n, pc, h, w, *tail) -> contiguous float32 (B, prod(tail))"""
    t = t.reshape((-1,) + tuple(tail))
    return t if (t.dtype is torch.float32 and t.is_contiguous()) else t.float().contiguous()      # (the renderer's outputs are: no call)


def _same_view(a, b):
    """True when a and b are the same values in the same memory (same storage offset, shape, strides, grad history)."""
    return a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype
                      and a._base is not None and a._base is b._base)


class LazyScalars(MutableMapping):
    """The loss dict of loss.py:219-229 ({name: python float}) without its synchronisation: the values are copied to pinned host memory
    asynchronously when the loss is computed and the host waits for that copy only when an entry is read (logging handlers read them
    every N iterations; a step whose dict nobody reads never stalls, and the backward is launched while the forward still runs).  A
    mutable Mapping: ``d["loss"]``, ``d.items()``, ``dict(d)``, ``d["x"] = 1.0``, ``d.update(...)`` behave like the reference's dict (the
    first access of any kind waits for the copy); pickling / ``copy.deepcopy`` (torch.save of an engine's output) yield a plain dict.
    It is NOT a ``dict`` subclass -- ``json.dumps`` walks a dict subclass' own storage behind its methods' back and would print the
    unmaterialised (empty) one: ``json.dumps(dict(d))`` is the spelling."""

    def __init__(self, keys, values: torch.Tensor):
        self._keys, self._vals = list(keys), None
        if values.is_cuda:
            self._host = torch.empty(values.shape, dtype=values.dtype, pin_memory=True)
            self._host.copy_(values, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record()
        else:
            self._host, self._event = values, None

    def _dict(self):
        if self._vals is None:
            if self._event is not None:
                self._event.synchronize()
            self._vals = dict(zip(self._keys, self._host.tolist()))
        return self._vals

    def __getitem__(self, k):
        return self._dict()[k]

    def __setitem__(self, k, v):
        self._dict()[k] = v

    def __delitem__(self, k):
        del self._dict()[k]

    def __iter__(self):
        return iter(self._keys if self._vals is None else self._vals)

    def __len__(self):
        return len(self._keys if self._vals is None else self._vals)

    def __reduce__(self):
        return (dict, (self._dict(),))

    def __repr__(self):
        return repr(self._dict())


class ReconstructionLoss:
    def __init__(self, config, use_automasking=False) -> None:
        self.criterion_str = config.get("criterion", "l2")
        if self.criterion_str not in ("l2", "l1", "l1+ssim"):
            raise ValueError(f"unknown criterion {self.criterion_str}")
        self.invalid_policy = config.get("invalid_policy", "strict")
        assert self.invalid_policy in ["strict", "weight_guided", "weight_guided_diverse", None, "none"]
        self.ignore_invalid = self.invalid_policy is not None and self.invalid_policy != "none"
        self.lambda_coarse = config.get("lambda_coarse", 1)
        self.lambda_fine = config.get("lambda_fine", 1)
        self.use_automasking = use_automasking
        self.lambda_entropy = config.get("lambda_entropy", 0)
        self.lambda_depth_reg = config.get("lambda_depth_reg", 0)
        self.lambda_alpha_reg = config.get("lambda_alpha_reg", 0)
        self.lambda_surfaceness_reg = config.get("lambda_surfaceness_reg", 0)
        self.lambda_edge_aware_smoothness = config.get("lambda_edge_aware_smoothness", 0)
        self.lambda_depth_smoothness = config.get("lambda_depth_smoothness", 0)
        self.median_thresholding = config.get("median_thresholding", False)
        self.alpha_reg_reduction = config.get("alpha_reg_reduction", "ray")
        self.alpha_reg_fraction = config.get("alpha_reg_fraction", 1 / 8)
        if self.alpha_reg_reduction not in ("ray", "slice"):
            raise ValueError(f"Unknown reduction for alpha regularization: {self.alpha_reg_reduction}")
        self._resolved = {}   # _mask_inputs' results of the call in flight (every scale reads scale 0's masks; one diverse-flags launch)
        self._lin = {}    # (scales, rays per scale, fine present, lambdas[, device]) -> the (9 x 3 S) matrix of loss_matrix()
        # opt-in (like native_mlp_color): criterion l1 / l2, median thresholding and weight_guided_diverse on bts_pixel_loss /
        # bts_loss_diverse_flags (csrc/bts_loss_pixel.hip)
        self.native_pixel_loss = bool(config.get("native_pixel_loss", False))
        self.diverse = self.invalid_policy == "weight_guided_diverse"
        self.pixel_criterion = self.criterion_str in ("l1", "l2")
        got = (f"criterion={self.criterion_str}, invalid_policy={self.invalid_policy}, automasking={use_automasking}, "
               f"median_thresholding={self.median_thresholding}")
        # opt-in: use_automasking on the loss kernels' _automask entry points (rgb_gt's fourth channel bounds every pixel's error)
        self.native_automask = bool(config.get("native_automask", False))
        if use_automasking and not self.native_automask:
            raise NotImplementedError("use_automasking=True runs on the HIP loss kernels' threshold variants with the config key "
                                      "`native_automask: true` (rgb_gt then carries automask.automask_images' error map as a fourth "
                                      "channel; the rendered rgb keeps 3); got " + got)
        # opt-in: l1+ssim with median thresholding on bts_photometric_loss_median (the median variant of the tiled passes)
        self.native_ssim_median = bool(config.get("native_ssim_median", False))
        self.ssim_median = self.criterion_str == "l1+ssim" and bool(self.median_thresholding)
        if self.ssim_median and not self.native_ssim_median:
            raise NotImplementedError("criterion 'l1+ssim' with median_thresholding=True runs on the HIP loss' median variant of the tiled "
                                      "passes with the config key `native_ssim_median: true`; got " + got)
        # opt-in: the regularisers (alpha_reg, surfaceness, entropy, depth_reg / depth_smoothness) on bts_loss_regularisers
        # (csrc/bts_loss_reg.hip) in place of the torch expressions of _call
        self.native_regularisers = bool(config.get("native_regularisers", False))
        if (self.pixel_criterion or self.diverse) and not self.native_pixel_loss:
            raise NotImplementedError("the fused HIP loss covers criterion 'l1+ssim' with invalid_policy strict / weight_guided / none, "
                                      "without automasking / median thresholding (every shipped config); criterion 'l1' / 'l2' (with or "
                                      "without median_thresholding) and invalid_policy 'weight_guided_diverse' run on their own HIP kernels "
                                      "with the config key `native_pixel_loss: true`; got " + got)

    @staticmethod
    def get_loss_metric_names():
        return ["loss", "loss_rgb_coarse", "loss_rgb_fine", "loss_ray_entropy", "loss_depth_reg"]

    def _split_gt(self, rgb_gt):
        """-> (colours (B, 3), threshold (B) | None): with automasking the fourth channel of rgb_gt is the per-ray bound (loss.py:139-143)"""
        if not self.use_automasking:
            return _flat(rgb_gt, (rgb_gt.shape[-1],)).detach(), None      # (3; C of a processed target, image_processor.PatchProcessor's 27)
        if rgb_gt.shape[-1] != 4:
            raise ValueError(f"use_automasking=True reads the error map as rgb_gt's fourth channel (automask.automask_images, a sampler "
                             f"with channels=4); got rgb_gt with {rgb_gt.shape[-1]} channels")
        return _flat(rgb_gt[..., :3], (3,)).detach(), _flat(rgb_gt[..., 3], ()).detach()

    @property
    def regularisers_on(self):
        """any optional regulariser's lambda > 0 (read per call: a schedule may change them)"""
        return (self.lambda_depth_reg > 0 or self.lambda_alpha_reg > 0 or self.lambda_surfaceness_reg > 0 or self.lambda_depth_smoothness > 0
                or self.lambda_entropy > 0)

    def _mask_keys(self, level0):
        """the entries of scale 0's render dict the invalid-ray policy reads (a fine dict that aliases them shares the coarse launch): the
        per-sample tensors of a full dict, the renderer's per-ray reductions of a lean one, all three per-sample tensors under diverse"""
        if not self.ignore_invalid:
            return ()
        if self.diverse:
            missing = [k for k in ("rgb_samps", "weights", "invalid") if k not in level0]
            if missing:
                raise KeyError("invalid_policy weight_guided_diverse reads the per-sample `rgb_samps`, `weights` and `invalid`, which this render "
                               f"dict does not carry (missing: {', '.join(missing)}): call the renderer with want_rgb_samps=True and "
                               "want_weights=True and without lean_training_outputs (NeRFRenderer drops the per-sample tensors in that mode)")
            return ("rgb_samps", "weights", "invalid")
        if "weights" not in level0:     # lean training outputs: the renderer's epilogue reduced weights / invalid per ray and view
            return ("invalid_wsum",) if self.invalid_policy == "weight_guided" else ("invalid_any",)
        return ("weights", "invalid") if self.invalid_policy == "weight_guided" else ("invalid",)

    def _mask_inputs(self, level0, per_sample=False):
        """Scale 0's render dict -> (the policy for the kernels, {weights, invalid, invalid_wsum, invalid_any[, rgb_samps]: flat tensor |
        None}) as the native entries take them by keyword: what _mask_keys names, flat (B, ...) and detached; a tensor the policy does not
        read is None (and never flattened).  Under diverse the kernels of l1+ssim and the regularisers get the per-(ray, view) flags
        (bts_loss_diverse_flags) as `invalid_any` of the strict policy, whose all_v(flag > .5) is the diverse rule -- they serve it
        unchanged; ``per_sample``: the three per-sample tensors themselves (native.pixel_loss, and the flags' own inputs).  Resolved once
        per render dict and call (every scale reads scale 0's: one flattening, one flags launch); the callers do not write to the result."""
        hit = self._resolved.get((id(level0), per_sample))
        if hit is not None and hit[0] is level0:
            return hit[1:]
        keys = self._mask_keys(level0)
        policy, masks = self.invalid_policy, dict.fromkeys(_MASKS if per_sample else _MASKS[:4])
        if self.diverse and not per_sample:
            m = self._mask_inputs(level0, per_sample=True)[1]
            policy, masks["invalid_any"] = "strict", native.loss_diverse_flags(m["rgb_samps"], m["weights"], m["invalid"])
        else:
            for k in keys:      # (n, pc, h, w, *tail) each; rgb_samps as (K, nv, 3) however the renderer folded its last two
                tail = level0[k].shape[4:] if k != "rgb_samps" else tuple(level0["invalid"].shape[4:]) + (3,)
                masks[k] = _flat(level0[k], tail).detach()
        self._resolved[(id(level0), per_sample)] = (level0, policy, masks)
        return policy, masks

    def _terms(self, fn, level, level0, gt, eas, per_sample=False, **kw):
        """-> (fn's three terms of one set of renderer outputs in patch layout as one (3,) tensor, number of rays).  gt: _split_gt's pair;
        kw: the entry's own keywords."""
        rgb_gt, thresh = gt
        rgb = level["rgb"]                                   # (n, pc, h, w, nv, 3)
        n, pc, h, w, nv, c = rgb.shape
        if c != 3:
            return self._terms_channels(level, level0, gt, eas)
        policy, masks = self._mask_inputs(level0, per_sample)
        kw.update(masks, rgb_gt=rgb_gt, patch_h=h, patch_w=w, invalid_policy=policy, eas=eas, thresh=thresh)
        terms = _NativeTerms.apply(fn, (0, 1), _flat(rgb, (nv * 3,)), _flat(level["depth"], ()) if eas else None, kw)
        return terms, n * pc * h * w

    def _terms_channels(self, level, level0, gt, eas):
        """_terms for other than 3 colour channels (the 27 of image_processor {type: patch}): criterion l1 / l2 on bts_pixel_loss_channels
        under none / strict / weight_guided; every other option names itself"""
        rgb_gt, thresh = gt
        rgb = level["rgb"]
        n, pc, h, w, nv, c = rgb.shape
        what = f"on {c} colour channels is not served (the HIP loss takes it on 3; on C channels: criterion l1 / l2, invalid_policy none / strict / weight_guided)"
        if not self.pixel_criterion:
            raise NotImplementedError(f"criterion 'l1+ssim' {what}")
        if self.median_thresholding:
            raise NotImplementedError(f"median_thresholding {what}")
        if self.diverse:
            raise NotImplementedError(f"invalid_policy 'weight_guided_diverse' {what}")
        if self.use_automasking or thresh is not None:
            raise NotImplementedError(f"use_automasking {what}")
        if eas:
            raise NotImplementedError(f"lambda_edge_aware_smoothness > 0 {what}; the reference itself raises there: its edge_aware_smoothness "
                                      "reshapes the target to 3 channels")
        policy, masks = self._mask_inputs(level0)
        kw = dict(masks, rgb_gt=rgb_gt, criterion=self.criterion_str, invalid_policy=policy)
        terms = _NativeTerms.apply(_pixel_c_terms, (0, 1), _flat(rgb, (nv * c,)), None, kw)
        return terms, n * pc * h * w

    def _sums(self, level, level0, gt, eas):
        """-> ((sum of the rgb term, sum of the smoothness term, number of invalid rays) as one (3,) tensor, number of rays): l1+ssim.  With
        median thresholding the same arguments go to the median entry with the number of batch samples (and come back as terms, the rgb
        one normalised by the kept count: _photometric)"""
        if self.ssim_median:
            return self._terms(_median_terms, level, level0, gt, eas, n=level["rgb"].shape[0])
        return self._terms(_photometric_sums, level, level0, gt, eas)

    def _pixel(self, level, level0, gt, eas):
        """-> (rgb term, sum of the smoothness term, number of invalid rays) as one (3,) tensor, number of rays: criterion l1 / l2"""
        return self._terms(_pixel_terms, level, level0, gt, eas, per_sample=True, n=level["rgb"].shape[0], criterion=self.criterion_str,
                           median=bool(self.median_thresholding))

    def _photometric(self, level, level0, gt, eas):
        """-> (mean rgb term, mean smoothness term, invalid-ray ratio)"""
        if self.pixel_criterion:
            terms, B = self._pixel(level, level0, gt, eas)
            return terms[0], terms[1] / B, terms[2] / B
        sums, B = self._sums(level, level0, gt, eas)
        if self.ssim_median:      # (the rgb term arrives as sum of kept e / count)
            return sums[0], sums[1] / B, sums[2] / B
        return sums[0] / B, sums[1] / B, sums[2] / B

    _KEYS = ["loss_rgb_coarse", "loss_rgb_fine", "loss_ray_entropy", "loss_depth_reg", "loss_alpha_reg", "loss_eas",
             "loss_depth_smoothness", "loss_invalid_ratio", "loss"]

    def _call_photometric_only(self, data):
        """The shipped configs' loss -- photometric term (coarse + the fine dict trainer.py:247-248 aliases to it) and edge-aware
        smoothness, no optional regulariser -- is LINEAR in the per-scale sums the HIP pass returns: loss and the whole logging dict are
        one (9 x 3 S) matrix applied to them.  The general path below spells the same algebra with ~25 zero-dimensional torch ops per
        scale (each a kernel launch, plus their autograd nodes and the zero fills of SelectBackward): ~190 launches and 0.5 ms of a
        3.7 ms exp_re10k.yaml step.  Returns None when the data needs the general path."""
        coarse_0, fine_0 = data["coarse"][0], data["fine"][0]
        S = len(data["coarse"])
        mask_keys = self._mask_keys(coarse_0)
        has_fine = []
        for coarse, fine in zip(data["coarse"], data["fine"]):
            if len(fine) > 0 and not (_same_view(fine["rgb"], coarse["rgb"]) and all(_same_view(fine_0[k], coarse_0[k]) for k in mask_keys)):
                return None
            has_fine.append(len(fine) > 0)
        eas_on = self.lambda_edge_aware_smoothness > 0
        gt = self._split_gt(data["rgb_gt"])       # (two tiny copies with automasking: rays, not pixels)
        sums, Bs = zip(*(self._sums(c, coarse_0, gt, eas_on) for c in data["coarse"]))
        st = torch.stack(sums).reshape(-1)                      # (3 S): rgb, eas, invalid count per scale
        M = self.loss_matrix(S, Bs, tuple(has_fine), st.device)
        loss = torch.dot(M[8], st)
        return loss, LazyScalars(self._KEYS, torch.mv(M, st.detach()))

    def loss_matrix(self, S, Bs, has_fine, device=None):
        """The (9 x 3 S) matrix that takes the per-scale sums [rgb term, smoothness term, invalid rays] of the HIP loss pass to the logging
        dict (rows in ``_KEYS`` order; row 8 = the loss).  Cached per (layout, lambdas): the reference reads ``self.lambda_*`` on every
        call, so a schedule that changes one of them gets a new matrix."""
        eas_on = self.lambda_edge_aware_smoothness > 0
        key = (S, tuple(Bs), tuple(has_fine), float(self.lambda_coarse), float(self.lambda_fine), float(self.lambda_edge_aware_smoothness))
        M = self._lin.get(key)
        if M is None:
            M = torch.zeros(9, 3 * S, dtype=torch.float64)
            for s in range(S):
                lam = self.lambda_coarse + self.lambda_fine if has_fine[s] else 1.0    # (without a fine dict the rgb term enters unscaled)
                M[0, 3 * s] = self.lambda_coarse / Bs[s]
                M[1, 3 * s] = (self.lambda_fine if has_fine[s] else 0) / Bs[s]
                M[5, 3 * s + 1] = 1.0 / Bs[s]
                M[8, 3 * s] = lam / Bs[s] / S
                M[8, 3 * s + 1] = (self.lambda_edge_aware_smoothness / 2 ** s if eas_on else 0) / Bs[s] / S
            M[7, 2] = 1.0 / Bs[0]
            M = self._lin[key] = M.float()
        if device is not None and device.type != "cpu":
            dkey = key + (device,)
            Md = self._lin.get(dkey)
            if Md is None:
                Md = self._lin[dkey] = M.to(device)
            return Md
        return M

    def _regularisers(self, coarse, coarse_0, scale, n_scales):
        """-> (6,) [alpha_reg, surfaceness, entropy, depth term, invalid rays, this scale's share of the loss] or None when no term is on
        at this scale: every regulariser whose lambda is > 0, one library call (``native_regularisers: true``).  The coefficients are
        read per call (a schedule may change the lambdas): lambda / n_scales, the entropy's undivided and at scale 0 only (the reference
        adds it after the division)."""
        on = lambda lam: float(lam) if lam > 0 else 0.0
        lam_depth = on(self.lambda_depth_reg) + on(self.lambda_depth_smoothness)
        coef = (on(self.lambda_alpha_reg) / n_scales, on(self.lambda_surfaceness_reg) / n_scales,
                on(self.lambda_entropy) if scale == 0 else 0.0, lam_depth / n_scales)
        if not any(c > 0 for c in coef):      # (the entropy alone: nothing to do at the scales behind the first)
            return None
        n, pc, h, w = coarse["depth"].shape
        alphas = _flat(coarse["alphas"], (coarse["alphas"].shape[-1],)) if (coef[0] > 0 or coef[1] > 0 or coef[2] > 0) else None
        depth = _flat(coarse["depth"], ()) if coef[3] > 0 else None
        if self.ignore_invalid and alphas is not None:
            policy, masks = self._mask_inputs(coarse_0)
        else:                                                    # (the depth term is never masked: alone it needs no keep flags)
            policy, masks = "none", dict.fromkeys(_MASKS[:4])
        return _NativeTerms.apply(_reg_terms, (5, 5), alphas, depth,
                                  dict(masks, rgb_samps=None, n=n, pc=pc, ph=h, pw=w, policy=policy, coef=coef,
                                       alpha_reg_reduction=self.alpha_reg_reduction, alpha_reg_fraction=float(self.alpha_reg_fraction)))

    def __call__(self, data):
        with profiler.record_function("loss_computation"):       # loss.py:84
            try:
                return self._call(data)
            finally:
                self._resolved.clear()

    def _call(self, data):
        if not self.pixel_criterion and not self.ssim_median and not self.regularisers_on:
            res = self._call_photometric_only(data)
            if res is not None:
                return res
        n_scales = len(data["coarse"])
        coarse_0, fine_0 = data["coarse"][0], data["fine"][0]
        dev = coarse_0["rgb"].device
        if "alphas" not in coarse_0 and (self.lambda_alpha_reg > 0 or self.lambda_surfaceness_reg > 0 or self.lambda_entropy > 0):
            raise KeyError("the alpha / surfaceness / entropy regularisers read the per-sample `alphas`, which this render dict does not "
                           "carry: call the renderer with want_alphas=True and without lean_training_outputs (NeRFRenderer drops the "
                           "per-sample tensors in that mode)")
        zero = torch.zeros((), device=dev)
        loss = zero
        gt = self._split_gt(data["rgb_gt"])
        m = dict(coarse=zero, fine=zero, depth_reg=zero, alpha_reg=zero, surf=zero, eas=zero, dsmooth=zero, inv=zero)
        keep_cache = None
        # `native_regularisers: true`: the blocks between the photometric term and the logging dict are one library call per scale
        native_reg = self.native_regularisers and self.regularisers_on
        reg, ent = None, zero

        def keep():   # 1 - invalid ray mask (n, pc, h, w) for the optional regularisers: the rule of the kernels' ray_invalid on _mask_inputs' tensors
            nonlocal keep_cache
            if keep_cache is None:
                policy, m = self._mask_inputs(coarse_0)
                if m["invalid_any"] is not None:             # strict on the renderer's reductions; the diverse flags
                    bad = torch.all(m["invalid_any"] > .5, dim=-1)
                elif m["invalid_wsum"] is not None:
                    bad = torch.all(m["invalid_wsum"] > .9, dim=-1)
                elif policy == "strict":
                    bad = torch.all(torch.any(m["invalid"] > .5, dim=-2), dim=-1)
                elif policy == "weight_guided":
                    bad = torch.all((m["invalid"] * m["weights"].unsqueeze(-1)).sum(-2) > .9, dim=-1)
                else:
                    bad = torch.zeros(coarse_0["depth"].numel(), dtype=torch.bool, device=dev)
                keep_cache = 1 - bad.reshape(coarse_0["depth"].shape).to(torch.float32)
            return keep_cache

        for scale in range(n_scales):
            coarse, fine = data["coarse"][scale], data["fine"][scale]
            eas_on = self.lambda_edge_aware_smoothness > 0
            rgb_loss, eas, inv_ratio = self._photometric(coarse, coarse_0, gt, eas_on)
            if scale == 0:
                m["inv"] = inv_ratio.detach()
            m["coarse"] = m["coarse"] + rgb_loss.detach() * self.lambda_coarse
            if len(fine) > 0:
                mask_keys = self._mask_keys(coarse_0)
                if _same_view(fine["rgb"], coarse["rgb"]) and all(_same_view(fine_0[k], coarse_0[k]) for k in mask_keys):
                    # trainer.py:247-248 aliases fine = dict(coarse): reconstruct() then views the SAME storage once per dict, so the
                    # tensors are different Python objects over identical memory -- one launch serves both terms
                    fine_loss = rgb_loss
                else:
                    fine_loss, _, _ = self._photometric(fine, fine_0, gt, False)
                m["fine"] = m["fine"] + fine_loss.detach() * self.lambda_fine
                rgb_loss = rgb_loss * self.lambda_coarse + fine_loss * self.lambda_fine
            loss = loss + rgb_loss

            if native_reg:
                if eas_on:
                    m["eas"] = m["eas"] + eas.detach()
                    loss = loss + eas * self.lambda_edge_aware_smoothness / (2 ** scale)
                out = self._regularisers(coarse, coarse_0, scale, n_scales)
                if out is None:
                    continue
                terms = out.detach()
                reg = out[5] if reg is None else reg + out[5]
                if self.lambda_depth_reg > 0:
                    m["depth_reg"] = m["depth_reg"] + terms[3]
                if self.lambda_depth_smoothness > 0:
                    m["dsmooth"] = m["dsmooth"] + terms[3]
                if self.lambda_alpha_reg > 0:
                    m["alpha_reg"] = m["alpha_reg"] + terms[0]
                if scale == 0 and self.lambda_entropy > 0:
                    ent = terms[2]
                continue
            if self.lambda_depth_reg > 0:
                d = coarse["depth"]
                s = ((d[:, :, 1:, :] - d[:, :, :-1, :]) ** 2).mean() + ((d[:, :, :, 1:] - d[:, :, :, :-1]) ** 2).mean()
                m["depth_reg"] = m["depth_reg"] + s.detach()
                loss = loss + s * self.lambda_depth_reg
            if self.lambda_alpha_reg > 0:
                a = coarse["alphas"]
                a_sum = a[..., :-1].sum(-1)
                cap = torch.ones_like(a_sum) * (a.shape[-1] * self.alpha_reg_fraction)
                if self.ignore_invalid:
                    a_sum, cap = a_sum * keep(), cap * keep()
                if self.alpha_reg_reduction == "ray":
                    s = (a_sum - cap).clamp_min(0)
                else:
                    s = (a_sum.sum(dim=-1) - cap.sum(dim=-1)).clamp_min(0) / a_sum.shape[-1]
                s = s.mean()
                m["alpha_reg"] = m["alpha_reg"] + s.detach()
                loss = loss + s * self.lambda_alpha_reg
            if self.lambda_surfaceness_reg > 0:
                a = coarse["alphas"]
                p = (-torch.log(torch.exp(-a.abs()) + torch.exp(-(1 - a).abs()))).mean(-1)
                if self.ignore_invalid:
                    p = p * keep()
                s = p.mean()
                m["surf"] = m["surf"] + s.detach()
                loss = loss + s * self.lambda_surfaceness_reg
            if eas_on:
                m["eas"] = m["eas"] + eas.detach()
                loss = loss + eas * self.lambda_edge_aware_smoothness / (2 ** scale)
            if self.lambda_depth_smoothness > 0:
                d = coarse["depth"]
                s = ((d[..., :-1, :] - d[..., 1:, :]) ** 2).mean() + ((d[..., :, :-1] - d[..., :, 1:]) ** 2).mean()
                m["dsmooth"] = m["dsmooth"] + s.detach()
                loss = loss + s * self.lambda_depth_smoothness

        loss = loss / n_scales
        if native_reg:
            loss = loss + reg
        elif self.lambda_entropy > 0:
            a = coarse_0["alphas"] + 1e-5
            dens = a / a.sum(dim=-1, keepdim=True)
            ent = (-(dens * torch.log(dens)).sum(-1) / math.log2(a.shape[-1]) * keep()).mean()
            loss = loss + ent * self.lambda_entropy

        # one device-to-host copy for the whole logging dict (the reference pays one synchronisation per entry), and not even that one
        # stalls the step: the copy is asynchronous, the host waits for it when somebody READS an entry (LazyScalars)
        vals = torch.stack([m["coarse"], m["fine"], ent.detach(), m["depth_reg"], m["alpha_reg"], m["eas"], m["dsmooth"], m["inv"],
                            loss.detach()])
        return loss, LazyScalars(self._KEYS, vals)
