"""The trainer's ``image_processor`` (models/bts/trainer.py:54-69, models/bts/model/image_processor.py): what turns the loader's frames
in [-1, 1] into the colour targets of the loss and the colour grid of the renderer.  Torch plumbing on any device, with the
reference's signatures, ``.channels`` and output.

``PatchProcessor(3)`` gives every pixel its 3 x 3 neighbourhood as 27 channels; handed to ``BTSNet.encode(images_alt=...)`` of a model
with ``native_patch_color: true`` the renderer returns 27 channels per view without ever sampling these frames (the HIP kernels of
csrc/bts_patch_color.hip read the packed RGB frames with a second clamp) -- the materialised tensor is what ``trainer.py`` indexes and
the ray samplers gather the targets from, as in the reference."""
import torch
import torch.nn.functional as F
from torch import nn


class RGBProcessor(nn.Module):
    """(n, v, 3, h, w) in [-1, 1] -> the same frames in [0, 1]."""
    channels = 3

    def forward(self, images):
        return images * .5 + .5


class PatchProcessor(nn.Module):
    """(n, v, 3, h, w) in [-1, 1] -> (n, v, 3 * patch_size^2, h, w) in [0, 1]: channel (y * patch_size + x) * 3 + c at pixel (i, j) is
    colour c at row clamp(i + y - patch_size // 2), column clamp(j + x - patch_size // 2) -- the frame padded by replication, cut at
    the patch_size^2 shifts.  An even patch_size fails in the final view, as it does in the reference."""

    def __init__(self, patch_size) -> None:
        super().__init__()
        self.patch_size = patch_size
        self.channels = 3 * patch_size ** 2

    def forward(self, images):
        n, v, c, h, w = images.shape
        ps, half = self.patch_size, self.patch_size // 2
        padded = F.pad(images.view(n * v, c, h, w) * .5 + .5, (half, half, half, half), mode="replicate")
        hp, wp = padded.shape[-2:]
        shifts = [padded[:, :, y:hp - (ps - 1 - y), x:wp - (ps - 1 - x)] for y in range(ps) for x in range(ps)]
        return torch.cat(shifts, dim=1).view(n, v, self.channels, h, w)


def _perceptual(config):
    raise NotImplementedError("image_processor type 'perceptual' needs LPIPS' VGG weights, which are not shipped; use 'rgb' or 'patch'")


_TYPES = {"rgb": lambda config: RGBProcessor(), "patch": lambda config: PatchProcessor(config.get("patch_size", 3)), "perceptual": _perceptual}


def make_image_processor(config):
    """The trainer's factory: ``{type: rgb | patch | perceptual[, patch_size: 3]}``, the type in any case, default RGB."""
    kind = config.get("type", "RGB").lower()
    if kind not in _TYPES:
        raise NotImplementedError(f"Unsupported image processor type: {kind}")
    return _TYPES[kind](config)
