"""Auto-masking (``use_automasking``): the trainer's error map (models/bts/trainer.py:201-206) on one HIP launch.

The reference compares every processed frame with every loss frame on whole frames (``compute_errors_l1ssim`` of .5 x frame against
.5 x loss frame, mean over the loss frames: about twenty torch ops on (n v L, 3, H + 2, W + 2) tensors) and concatenates the result to the
frames as a fourth channel, which the samplers then carry into ``rgb_gt`` and the loss uses as a per-pixel bound on the photometric
error (``ReconstructionLoss(conf, use_automasking=True)`` with ``native_automask: true``).  ``bts_automask_errors``
(csrc/bts_automask.hip) reads every input plane once and writes map and concatenation in the same launch.

    images_ip = automask_images(images_ip, ids_loss, len(ids_render))        # trainer.py:203-206
    net.encode(images, projs, poses, ids_encoder=..., ids_render=ids_render, images_alt=images_ip)
    all_rays, all_rgb_gt = sampler.sample(images_ip[:, ids_loss], ...)       # a sampler built with channels=4

Quirks of the reference kept on purpose (include/bts_render.h): the frames, already in [0, 1], are halved a second time; the partners
are the LOSS frames although the trainer calls them ``render_imgs`` (its ``.view`` only works when both lists are equally long:
``n_render``); a loss frame's comparison with itself (~ 0) is part of its mean.  There is no CPU fallback."""
import torch

from . import native
from ._lib import BTS_MAX_VIEWS

SCALE = .5      # trainer.py:203-204


def _ids(images_ip, ids_loss, n_render):
    if not isinstance(images_ip, torch.Tensor) or images_ip.dim() != 5 or images_ip.shape[2] != 3:
        raise ValueError(f"images_ip: expected the processed frames (n, v, 3, h, w), got {tuple(getattr(images_ip, 'shape', ()))}")
    ids = [int(i) for i in (ids_loss.tolist() if isinstance(ids_loss, torch.Tensor) else ids_loss)]
    if n_render is not None and int(n_render) != len(ids):
        raise ValueError(f"automasking compares every frame with the {len(ids)} loss frames but the reference views the result with "
                         f"len(ids_render) = {int(n_render)} (trainer.py:203-204): the two counts must be equal")
    v = images_ip.shape[1]
    if not 1 <= len(ids) <= BTS_MAX_VIEWS or any(i < 0 or i >= v for i in ids):
        raise ValueError(f"ids_loss: expected 1 .. {BTS_MAX_VIEWS} frame indices in [0, {v}), got {ids}")
    return ids


def _frames(images_ip):
    """(a CPU tensor goes on as it is: native refuses it)"""
    x = images_ip.detach()
    return x.float().contiguous() if x.is_cuda else x


def automask_errors(images_ip, ids_loss, n_render=None):
    """images_ip (n, v, 3, h, w) in [0, 1], ids_loss -> (n, v, 1, h, w): trainer.py:203-205's ``errors``"""
    ids = _ids(images_ip, ids_loss, n_render)
    errors, _ = native.automask_errors(_frames(images_ip), ids, SCALE, want_errors=True, want_images4=False)
    return errors.unsqueeze(2)


def automask_images(images_ip, ids_loss, n_render=None):
    """images_ip (n, v, 3, h, w) in [0, 1], ids_loss -> (n, v, 4, h, w): trainer.py:206's ``torch.cat((images_ip, errors), dim=2)``"""
    ids = _ids(images_ip, ids_loss, n_render)
    _, images4 = native.automask_errors(_frames(images_ip), ids, SCALE, want_errors=False, want_images4=True)
    return images4
