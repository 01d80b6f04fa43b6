"""The trainer's ``visualize`` (models/bts/trainer.py:430-506) on the HIP kernels of csrc/bts_train_vis.hip: the eight panels it logs for
the first six rendered frames of batch element 0 -- input, reconstruction, colour-mapped depth per scale, the depth profile of three
image rows, ray entropy, alpha sum, reconstruction error, invalid share -- from ONE library call (``bts_train_vis``, two launches) that
reads the render dict where it lies and synchronises nothing.  ``visualize`` keeps the reference's signature, so the trainer binds with

    from behindthescenes_amd.train_vis import visualize

Grid assembly (``make_grid``), TensorBoard's byte conversion and the copies to the host stay with the caller.  The reference's in-place
``alphas += 1e-5`` on the render dict is deliberately NOT reproduced: the inputs are bit-identical after the call, the outputs are
unaffected.  There is no torch fallback: CPU tensors are rejected, as everywhere else in this package."""
import torch

from . import native
from ._lib import BtsNativeError
from .novel_views import _device_table

PANELS = ("input_im", "recon_im", "recon_depth", "depth_profile", "ray_entropy", "alpha_sum", "recon_mse", "invalids")
FIELDS = ("f_depth", "f_profile", "f_entropy", "f_alpha_sum", "f_mse", "f_invalid")


def _first(x, name):
    """batch element 0 of a tensor of the render dict, contiguous (a slice [0] of a contiguous tensor is: no copy)"""
    if not isinstance(x, torch.Tensor):
        raise BtsNativeError(f"{name}: expected a tensor")
    if not x.is_cuda:
        raise BtsNativeError(f"{name}: must live on the GPU (got {x.device}); the HIP panels have no CPU path")
    return x.detach()[0].float().contiguous()


def vis_panels(data, cmap="plasma", fields=False):
    """``data``: the trainer's output dict -- ``imgs`` (a list of ``(n, 3, h, w)``), ``fine[s]["rgb" | "depth"]``,
    ``coarse[0]["alphas" | "invalid"]``, ``z_near``, ``z_far`` (what ``FusedEvalFrame`` returns plus the three keys the trainer adds).
    -> the panels under the reference's tags: ``input_im``, ``recon_im``, ``recon_depth_0`` ..., ``depth_profile``, ``ray_entropy``,
    ``alpha_sum``, ``recon_mse``, ``invalids``; with ``fields`` also the scalar fields before the colour map (``f_depth_0`` ...,
    ``f_profile``, ``f_entropy``, ``f_alpha_sum``, ``f_mse``, ``f_invalid``).  One library call, nothing synchronises: ``z_near`` /
    ``z_far`` may be numbers or the trainer's device tensors, which the kernel reads itself."""
    coarse, fine = data["coarse"][0], data["fine"]
    if coarse.get("alphas") is None:
        raise KeyError("alphas: the visualisation needs the coarse pass's alphas -- ask the renderer for them (want_alphas=True, "
                       "without lean_training_outputs)")
    if coarse.get("invalid") is None:
        raise KeyError("invalid: the visualisation needs the coarse pass's invalid flags (want_invalid)")
    alphas, invalid = _first(coarse["alphas"], "alphas"), _first(coarse["invalid"], "invalid")
    if alphas.dim() != 4:
        raise BtsNativeError(f"alphas: (n, v, h, w, K) expected -- the sampler's reconstruct() output, got {tuple(coarse['alphas'].shape)}")
    v, h, w, K = (int(s) for s in alphas.shape)
    imgs = list(data["imgs"])
    if len(imgs) != v:
        raise BtsNativeError(f"imgs holds {len(imgs)} frames, the render dict {v}: the panels pair them one to one (the reference "
                             "breaks there too)")
    T = min(v, 6)
    imgs = [_first(i, f"imgs[{j}]") for j, i in enumerate(imgs[:T])]
    rgb = _first(fine[0]["rgb"], "rgb")
    rgb = rgb.reshape(v, h, w, -1, 3)               # trainer.py:456's view
    depths = [_first(f["depth"], f"fine[{s}].depth").reshape(v, h, w) for s, f in enumerate(fine)]
    N, lut, _ = _device_table(cmap, alphas.device)
    out = native.train_vis(imgs, rgb, depths, alphas, invalid, data["z_near"], data["z_far"], N, lut, fields=fields)
    panels = {}
    for k in PANELS:
        if k == "recon_depth":
            for s in range(len(depths)):
                panels[f"recon_depth_{s}"] = out[k][s]
        else:
            panels[k] = out[k]
    if fields:
        for s in range(len(depths)):
            panels[f"f_depth_{s}"] = out["f_depth"][s]
        for k in FIELDS[1:]:
            panels[k] = out[k]
    return panels


def _tags(panels):
    """the reference's order of add_image calls (trainer.py:498-506)"""
    depths = sorted((k for k in panels if k.startswith("recon_depth_")), key=lambda k: int(k.rsplit("_", 1)[1]))
    return ["input_im", "recon_im"] + depths + ["depth_profile", "ray_entropy", "alpha_sum", "recon_mse", "invalids"]


def visualize(engine, logger, step, tag, make_grid=None):
    """trainer.py:430-506 with its signature: ``engine.state.output["output"]`` -> ``vis_panels`` -> ``make_grid(panel, nrow=int(T **
    .5))`` -> ``logger.writer.add_image(f"{tag}/<name>", grid.cpu(), global_step=step)`` in the reference's order.  ``make_grid``:
    torchvision's by default (imported here, when first needed)."""
    if make_grid is None:
        try:
            from torchvision.utils import make_grid
        except ImportError as e:
            raise BtsNativeError("visualize: torchvision is not installed; pass make_grid= (any callable (panel, nrow=) -> image)") from e
    print("Visualizing")
    data = engine.state.output["output"]
    writer = logger.writer
    panels = vis_panels(data)
    nrow = int(panels["input_im"].shape[0] ** .5)
    names = _tags(panels)
    grids = [make_grid(panels[name], nrow=nrow) for name in names]      # every grid first, as there (:489-496)
    for name, grid in zip(names, grids):
        writer.add_image(f"{tag}/{name}", grid.cpu(), global_step=step)
