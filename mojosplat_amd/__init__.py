"""mojosplat_amd -- MI355X (gfx950) backend for the mojosplat 3D-Gaussian-splatting render path.

Public surface = the reference's (mojosplat/render.py, projection.py, binning.py,
rasterization.py, utils.py): ``render_gaussians``, ``Camera``, ``project_gaussians``,
``bin_gaussians_to_tiles``, ``rasterize_gaussians``, each with a ``backend=`` switch that gains
``"hip"``.  Importing this package needs neither a GPU nor the built library.
"""
from .utils import Camera, look_at
from .projection import project_gaussians
from .binning import bin_gaussians_to_tiles
from .rasterization import rasterize_gaussians
from .render import render_gaussians, render_gaussians_batch, TILE_SIZE
from .sh import evaluate_sh
from .densify import DensifyStats
from .loss import photometric_loss, ssim
from .optim import GaussianAdam
from .refine import densify_and_prune, reset_opacities, DensifyResult
from .mcmc import relocate_dead, grow, inject_noise, McmcResult
from .knn import knn, init_from_points, scene_extent
from .sceneio import save_ply, load_ply, pack_ply_rows, unpack_ply_rows, ply_header, parse_ply_header, PlyLayout
from .splatio import (compress_scene, decompress_scene, save_compressed_ply, load_compressed_ply, save_splat, load_splat,
                      CompressedScene)
from .bilagrid import bilagrid_identity, bilagrid_slice, bilagrid_tv_loss, bilagrid_slice_torch, bilagrid_tv_loss_torch
from .contrib import (ContributionStats, contributions_from_lists, accumulate_contributions, select_by_contribution, lift_mask,
                      prune_scene)
from .edit import sh_rotation_matrices, transform_scene, transform_camera, crop_scene, merge_scenes


def prepare_scene(*args, **kw):
    """Sort a scene along a Morton curve and compute its block bounds for the multi-GPU band path: scene_order.prepare_scene."""
    from .scene_order import prepare_scene as _prepare
    return _prepare(*args, **kw)


def release_scratch():
    """Give the calling thread's cached render scratch (and the shared lanes') back to the allocator: _fused.release_scratch."""
    from ._fused import release_scratch as _release
    _release()

__all__ = ["Camera", "look_at", "project_gaussians", "bin_gaussians_to_tiles",
           "rasterize_gaussians", "render_gaussians", "render_gaussians_batch", "evaluate_sh", "DensifyStats", "photometric_loss", "ssim", "GaussianAdam", "densify_and_prune", "reset_opacities", "DensifyResult", "relocate_dead", "grow", "inject_noise", "McmcResult", "knn", "init_from_points", "scene_extent", "save_ply", "load_ply", "pack_ply_rows", "unpack_ply_rows", "ply_header", "parse_ply_header", "PlyLayout", "compress_scene", "decompress_scene", "save_compressed_ply", "load_compressed_ply", "save_splat", "load_splat", "CompressedScene", "sh_rotation_matrices", "transform_scene", "transform_camera", "crop_scene", "merge_scenes", "bilagrid_identity", "bilagrid_slice", "bilagrid_tv_loss", "bilagrid_slice_torch", "bilagrid_tv_loss_torch", "ContributionStats", "contributions_from_lists", "accumulate_contributions", "select_by_contribution", "lift_mask", "prune_scene", "release_scratch", "prepare_scene", "TILE_SIZE"]
