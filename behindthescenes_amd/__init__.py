"""behindthescenes_amd -- MI355X-native density-field renderer behind the reference's (Brummi/BehindTheScenes) Python
interfaces.  The computation lives in libbts_render.so (hand-written HIP for gfx950); see include/bts_render.h."""
from ._lib import BtsNativeError  # noqa: F401
from . import parallel, torch_modes  # noqa: F401
from .backbone import FeatureMapEncoder, make_backbone, register_backbone  # noqa: F401
from .code import PositionalEncoding  # noqa: F401
from .field import BTSNet  # noqa: F401
from .loss import ReconstructionLoss  # noqa: F401
from .mlp import ResnetBlockFC, ResnetFC, make_mlp  # noqa: F401
from .projection import distance_to_z  # noqa: F401
from .ray_sampler import ImageRaySampler, PatchRaySampler, RandomRaySampler, gen_rays  # noqa: F401
from .renderer import NeRFRenderer, _RenderWrapper  # noqa: F401
from .train_step import FusedEvalFrame, FusedTrainStep  # noqa: F401
from . import lidar_occupancy  # noqa: F401
from .lidar_occupancy import FusedOccupancyEval  # noqa: F401
from . import depth_metrics  # noqa: F401
from .depth_metrics import FusedDepthEval, compute_depth_metrics  # noqa: F401
from . import lidar_depth  # noqa: F401
from .lidar_depth import load_depth, load_depth_batch  # noqa: F401
from . import nvs_metrics  # noqa: F401
from .nvs_metrics import FusedNVSEval, compute_nvs_metrics  # noqa: F401
from . import bbox_occupancy  # noqa: F401
from .bbox_occupancy import FusedBBoxOccupancyEval  # noqa: F401
from . import novel_views  # noqa: F401
from .novel_views import FusedNovelViews, color_tensor, colorize_u8, pack_u8, render_poses  # noqa: F401
from . import automask  # noqa: F401
from .automask import automask_errors, automask_images  # noqa: F401
from . import train_vis  # noqa: F401
from . import image_processor  # noqa: F401
from .image_processor import PatchProcessor, RGBProcessor, make_image_processor  # noqa: F401
from .train_vis import vis_panels, visualize  # noqa: F401

__all__ = ["BTSNet", "NeRFRenderer", "PositionalEncoding", "ResnetFC", "ResnetBlockFC", "make_mlp", "make_backbone",
           "ImageRaySampler", "PatchRaySampler", "RandomRaySampler", "gen_rays", "distance_to_z", "ReconstructionLoss", "FusedTrainStep", "FusedEvalFrame", "FusedOccupancyEval", "lidar_occupancy", "FusedDepthEval", "compute_depth_metrics", "depth_metrics", "lidar_depth", "load_depth", "load_depth_batch", "FusedNVSEval", "compute_nvs_metrics", "nvs_metrics", "FusedBBoxOccupancyEval", "bbox_occupancy", "FusedNovelViews", "color_tensor", "colorize_u8", "pack_u8", "render_poses", "novel_views", "automask", "automask_errors", "automask_images", "train_vis", "vis_panels", "visualize", "image_processor", "make_image_processor", "RGBProcessor", "PatchProcessor", "BtsNativeError"]
