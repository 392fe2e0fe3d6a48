"""ctypes binding of libmojosplat_hip.so (the C ABI declared in include/mojosplat_hip.h).

This replaces the reference's plugin mechanism -- ``CustomOpLibrary(kernels_dir)`` created at
import time (reference mojosplat/projection.py:12-13, rasterization.py:9-10).  Differences by
design: the library is loaded lazily on the first ``backend="hip"`` call (so importing the
package works on a box with no GPU), it is a prebuilt gfx950 shared object rather than a
JIT-specialised kernel per (N, W, H, M) (projection.py:429-436, rasterization.py:169-179),
and a missing library or GPU is a hard error: there is no CPU fallback behind ``"hip"``.
"""
import ctypes
import os
from ctypes import c_float, c_int, c_int64, c_size_t, c_void_p

import torch

# MOJOSPLAT_HIP_LIB: another build of the same library (the -DMS_DIAG one of scripts/raster_waves.py)
_LIB_PATH = os.environ.get("MOJOSPLAT_HIP_LIB") or \
    os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libmojosplat_hip.so")
_lib = None

ABI_VERSION = 5

# name -> (restype, argtypes); mirrors include/mojosplat_hip.h one to one
_SIGNATURES = {
    "ms_version": (c_int, []),
    "ms_last_error_string": (ctypes.c_char_p, []),
    "ms_project_gaussians_fwd": (c_int, [c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                         c_void_p, c_float, c_float, c_float, c_float, c_int, c_int,
                                         c_float, c_float, c_float, c_float, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p]),
    "ms_isect_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "ms_isect_tiles_count": (c_int, [c_int64, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                     c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ms_isect_tiles_emit": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                    c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_int, c_int, c_float, c_float,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ms_project_isect_count": (c_int, [c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float,
                                       c_float, c_float, c_float, c_int, c_int, c_float, c_float, c_float,
                                       c_float, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ms_isect_offset_encode": (c_int, [c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "ms_rasterize_to_pixels_3dgs_fwd": (c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int,
                                                c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                                c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_void_p]),
    "ms_rasterize_to_pixels_3dgs_bwd": (c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int,
                                                c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_size_t, c_int, c_void_p]),
    "ms_rasterize_bwd_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "ms_render_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "ms_render_isect_bytes": (c_size_t, [c_int64, c_int]),
    "ms_render_fwd": (c_int, [c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                              c_void_p, c_float, c_float, c_float, c_float, c_int, c_int, c_float, c_float,
                              c_float, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t,
                              c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ms_render_workspace_layout": (c_int, [c_int64, c_int, c_int, c_void_p]),
    "ms_render_front_count_offset": (c_int, [c_int64, c_int, c_int, c_void_p]),
    "ms_render_bwd_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "ms_config_depth_cut": (c_int, [c_int, ctypes.c_longlong]),
    "ms_config_fused_sort": (c_int, [c_int]),
    "ms_render_redo_counts": (c_int, [c_void_p, c_size_t, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "ms_render_bwd": (c_int, [c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_float,
                              c_float, c_float, c_float, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_size_t,
                              c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "ms_isect_tiles_emit_speculative": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                                c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_int64,
                                                c_void_p, c_int, c_int, c_float, c_float, c_void_p, c_void_p,
                                                c_void_p]),
    "ms_spherical_harmonics_fwd": (c_int, [c_int64, c_int, c_int, c_void_p, c_float, c_float, c_float, c_void_p,
                                           c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "ms_spherical_harmonics_bwd": (c_int, [c_int64, c_int, c_int, c_void_p, c_float, c_float, c_float, c_void_p,
                                           c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ms_project_gaussians_bwd": (c_int, [c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                         c_float, c_float, c_float, c_float, c_int, c_int, c_float,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
}



class ViewLane(ctypes.Structure):
    """ms_view_lane (include/mojosplat_hip.h): one scratch set of ms_render_fwd_batch."""
    _fields_ = [("workspace", c_void_p), ("workspace_bytes", c_size_t), ("isect_buf", c_void_p),
                ("isect_bytes", c_size_t), ("host_info", c_void_p), ("sync_event", c_void_p), ("stream", c_void_p)]


_SIGNATURES["ms_render_fwd_batch"] = (c_int, [c_int, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                              c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float,
                                              c_int, c_void_p, c_int, ctypes.POINTER(ViewLane), c_int, c_void_p,
                                              c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_size_t),
                                              ctypes.POINTER(c_int)])

class Scene(ctypes.Structure):
    """ms_scene (include/mojosplat_hip.h): the Gaussians, marshalled once per scene (+ a prepared scene's block bounds)."""
    _fields_ = [("N", c_int64), ("means3d", c_void_p), ("scales", c_void_p), ("scales_are_log", c_int), ("quats", c_void_p),
                ("opacities", c_void_p), ("colors", c_void_p), ("color_dtype", c_int), ("CDIM", c_int),
                ("block_bounds", c_void_p), ("block_size", c_int), ("n_blocks", c_int64)]


class BandLane(ctypes.Structure):
    """ms_band_lane: one scratch set + the stream a band runs on + the two events that order it against the caller's."""
    _fields_ = [("workspace", c_void_p), ("workspace_bytes", c_size_t), ("isect_buf", c_void_p), ("isect_bytes", c_size_t),
                ("host_info", c_void_p), ("sync_event", c_void_p), ("stream", c_void_p), ("in_event", c_void_p),
                ("out_event", c_void_p)]


class BandFrame(ctypes.Structure):
    """ms_band_frame: one rank's band of one frame."""
    _fields_ = [("scene", ctypes.POINTER(Scene)), ("viewmat", c_void_p), ("fx", c_float), ("fy", c_float), ("cx", c_float),
                ("cy", c_float), ("W", c_int), ("H", c_int), ("eps2d", c_float), ("near_plane", c_float), ("far_plane", c_float),
                ("tile_size", c_int), ("row_begin", c_int), ("row_end", c_int), ("flags", c_int), ("backgrounds", c_void_p),
                ("render_colors", c_void_p), ("stage_events", c_void_p)]


_SIGNATURES["ms_render_bwd_rows_bytes"] = (c_size_t, [c_int64])
_SIGNATURES["ms_render_bwd_rows"] = (c_int, [c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p,
                                             c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p])
_SIGNATURES["ms_render_bwd_finish"] = (c_int, [c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_float, c_float,
                                               c_float, c_float, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p])
_SIGNATURES["ms_render_bwd_finish_densify"] = (c_int, [c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_float,
                                                       c_float, c_float, c_float, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                                       c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                                       c_void_p])
# the pose-gradient twins (include/mojosplat_hip.h): the namesake's arguments, then v_viewmat / v_campos, scratch, its bytes
_SIGNATURES["ms_pose_scratch_bytes"] = (c_size_t, [c_int64])
for _name in ("ms_project_gaussians_bwd", "ms_render_bwd_finish", "ms_render_bwd_finish_densify", "ms_render_bwd",
              "ms_spherical_harmonics_bwd"):
    _r, _a = _SIGNATURES[_name]
    _SIGNATURES[_name + "_pose"] = (_r, _a[:-1] + [c_void_p, c_void_p, c_size_t, c_void_p])
_SIGNATURES["ms_densify_stats_update"] = (c_int, [c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p])
_SIGNATURES["ms_scene_block_bounds_bytes"] = (c_size_t, [c_int64, c_int])
_SIGNATURES["ms_scene_prepare"] = (c_int, [c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p])
_SIGNATURES["ms_render_band_begin"] = (c_int, [ctypes.POINTER(BandFrame), ctypes.POINTER(BandLane), c_void_p])
_SIGNATURES["ms_render_band_finish"] = (c_int, [ctypes.POINTER(BandFrame), ctypes.POINTER(BandLane), c_void_p, c_int,
                                               ctypes.POINTER(c_int64)])

# the L1 + D-SSIM training loss (csrc/loss.hip): B, H, W, C, img, target, lambda, workspace, its bytes, ...
_SIGNATURES["ms_photometric_loss_workspace_bytes"] = (c_size_t, [c_int, c_int, c_int, c_int, c_int])
_SIGNATURES["ms_photometric_loss_fwd"] = (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_size_t,
                                                  c_int, c_void_p, c_void_p])
_SIGNATURES["ms_photometric_loss_bwd"] = (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_size_t,
                                                  c_void_p, c_void_p, c_void_p])



class AdamTensor(ctypes.Structure):
    """ms_adam_tensor (include/mojosplat_hip.h): one parameter tensor of an ms_adam_step call."""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p),
                ("rows", c_int64), ("width", c_int64), ("lr", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("bias_correction1", ctypes.c_double),
                ("bias_correction2_sqrt", ctypes.c_double)]


ADAM_MAX_TENSORS = 8
# the Adam step (csrc/adam.hip): n_tensors, the records (host), the visibility mask or None, its rows, stream
_SIGNATURES["ms_adam_step"] = (c_int, [c_int, ctypes.POINTER(AdamTensor), c_void_p, c_int64, c_void_p])


class DensifyRules(ctypes.Structure):
    """ms_densify_rules (include/mojosplat_hip.h): the float32 thresholds of ms_densify_classify; +inf = the rule is off."""
    _fields_ = [("grow_grad2d", c_float), ("log_grow", c_float), ("grow_radius", c_float), ("thr_opa", c_float),
                ("log_big", c_float), ("prune_radius", c_float)]


class DensifyTensor(ctypes.Structure):
    """ms_densify_tensor: one tensor of an ms_densify_move call."""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("width", c_int64), ("kind", c_int)]


DENSIFY_ROWS = 256            # MS_DENSIFY_ROWS: Gaussians per workgroup of the classify and move kernels
DENSIFY_SCAN_SPAN = 512       # MS_DENSIFY_SCAN_SPAN: workgroup counts per pass of the scan kernel's lanes
DENSIFY_MAX_TENSORS = 16
DENSIFY_COPY, DENSIFY_MEAN, DENSIFY_SCALE, DENSIFY_MOMENT = range(4)
# the densification step (csrc/densify.hip): classify + scan, then the table-driven move
_SIGNATURES["ms_densify_workspace_bytes"] = (c_size_t, [c_int64])
_SIGNATURES["ms_densify_classify"] = (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              ctypes.POINTER(DensifyRules), c_void_p, c_size_t, c_void_p, c_void_p])
_SIGNATURES["ms_densify_move"] = (c_int, [c_int64, c_int64, c_int64, c_int64, c_void_p, c_size_t, c_int,
                                          ctypes.POINTER(DensifyTensor), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p])


class McmcTensor(ctypes.Structure):
    """ms_mcmc_tensor: one tensor of an ms_mcmc_apply call, updated in place."""
    _fields_ = [("base", c_void_p), ("width", c_int64), ("kind", c_int)]


MCMC_ROWS = 256               # MS_MCMC_ROWS: Gaussians (or draws) per workgroup
MCMC_MAX_RATIO = 51           # MS_MCMC_MAX_RATIO: the relocation formula's largest n
MCMC_MAX_TENSORS = 16
MCMC_COPY, MCMC_OPACITY, MCMC_SCALE, MCMC_MOMENT = range(4)
# the MCMC strategy (csrc/mcmc.hip): sample (classify, scan, draw), the table-driven apply, the noise step
_SIGNATURES["ms_mcmc_workspace_bytes"] = (c_size_t, [c_int64])
_SIGNATURES["ms_mcmc_sample"] = (c_int, [c_int64, c_void_p, c_int, c_float, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                         c_size_t, c_void_p, c_void_p, c_void_p, c_void_p])
_SIGNATURES["ms_mcmc_apply"] = (c_int, [c_int64, c_int64, c_int64, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_int,
                                        ctypes.POINTER(McmcTensor), c_void_p, c_void_p, c_void_p, c_int, ctypes.c_double,
                                        c_void_p])
_SIGNATURES["ms_mcmc_noise"] = (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_float,
                                        c_float, c_void_p])

KNN_BLOCK = 64                # MS_KNN_BLOCK: points per bounding box = queries per wave
KNN_MAX_K = 8
# exact k nearest neighbours (csrc/knn.hip): N, points, order or None, k, dist2, idx or None, workspace, stream
_SIGNATURES["ms_knn_workspace_bytes"] = (c_size_t, [c_int64, c_int])
_SIGNATURES["ms_knn"] = (c_int, [c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p])


class PlyColumn(ctypes.Structure):
    """ms_ply_column (include/mojosplat_hip.h): file column <-> (tensor, float offset in its row), or no tensor."""
    _fields_ = [("tensor", c_int), ("offset", c_int), ("column", c_int)]


PLY_ROWS = 64                 # MS_PLY_ROWS: rows per workgroup
PLY_TENSORS = 5
PLY_MAX_COLUMNS = 128
PLY_MAX_STRIDE = 192
PLY_NONE = -1
# scene files (csrc/sceneio.hip): N, F, [S, rows,] tensors (host array of 5), widths (host), the table (host), [rows,] stream
_SIGNATURES["ms_ply_pack"] = (c_int, [c_int64, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_int), ctypes.POINTER(PlyColumn),
                                      c_void_p, c_void_p])
_SIGNATURES["ms_ply_unpack"] = (c_int, [c_int64, c_int, c_int, c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_int),
                                        ctypes.POINTER(PlyColumn), c_void_p])

SPLAT_CHUNK = 256             # MS_SPLAT_CHUNK: Gaussians per chunk of a compressed PLY = rows per workgroup
SPLAT_MAX_K = 25
# viewer formats (csrc/splatio.hip): N, K, [chunk_floats,] the prepared arrays and the file's elements (inputs first), stream
_SIGNATURES["ms_splat_compress"] = (c_int, [c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p])
_SIGNATURES["ms_splat_decompress"] = (c_int, [c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p])
# ... and the .splat row: N, pos, scale_lin, rgba, rot, rows, stream / N, rows, pos, scale_lin, rgba, rot, stream
_SIGNATURES["ms_splat32_pack"] = (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p])
_SIGNATURES["ms_splat32_unpack"] = (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p])


class Transform(ctypes.Structure):
    """ms_transform (include/mojosplat_hip.h): the float32 constants of a similarity transform, 181 floats."""
    _fields_ = [("A", c_float * 9), ("t", c_float * 3), ("r", c_float * 4), ("l", c_float),
                ("M1", c_float * 9), ("M2", c_float * 25), ("M3", c_float * 49), ("M4", c_float * 81)]


TRANSFORM_ROWS = 64           # MS_TRANSFORM_ROWS: Gaussians per workgroup of ms_scene_transform, K > 1
TRANSFORM_ROWS_K1 = 256       # MS_TRANSFORM_ROWS_K1: ... K = 1
# scene editing (csrc/transform.hip): N, K, means, scales, quats, features, the transform (host), the four outputs, stream
_SIGNATURES["ms_scene_transform"] = (c_int, [c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(Transform),
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p])

# bilateral-grid colour correction (csrc/bilagrid.hip): B, H, W, L, Gh, Gw, grids, img, ... / B, L, Gh, Gw, grids, ...
_SIGNATURES["ms_bilagrid_slice_workspace_bytes"] = (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int])
_SIGNATURES["ms_bilagrid_slice_fwd"] = (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p])
_SIGNATURES["ms_bilagrid_slice_bwd"] = (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_size_t, c_void_p, c_void_p, c_void_p])
_SIGNATURES["ms_bilagrid_tv_workspace_bytes"] = (c_size_t, [c_int, c_int, c_int, c_int])
_SIGNATURES["ms_bilagrid_tv_fwd"] = (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p])
_SIGNATURES["ms_bilagrid_tv_bwd"] = (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p])

# contribution statistics (csrc/contrib.hip): N, M, means2d, conics, opacities, tile_ranges, ids, weights or None, W, H,
# tile_size, pixels, max_weight, sum_q, wsum_q or None, stream
CONTRIB_FIXED_ONE = 1 << 30   # MS_CONTRIB_FIXED_ONE: units of the fixed-point sums
_SIGNATURES["ms_contrib_accumulate"] = (c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                                c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p])

# entry points added after ABI v1's first cut; bound when present
_OPTIONAL = {}

EXPORTS = tuple(_SIGNATURES)


class HipBackendError(RuntimeError):
    pass


def library_path() -> str:
    return _LIB_PATH


def load():
    """Load and type the shared library (no GPU needed for this step)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise HipBackendError(
            f"{_LIB_PATH} not found: build it with `python -m mojosplat_amd.csrc.build` "
            "(hipcc --offload-arch=gfx950). backend='hip' has no fallback.")
    L = ctypes.CDLL(_LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if the ABI is incomplete
        fn.restype, fn.argtypes = res, args
    for name, (res, args) in _OPTIONAL.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    if L.ms_version() != ABI_VERSION:
        raise HipBackendError(f"ABI mismatch: library {L.ms_version()} != binding {ABI_VERSION}")
    _lib = L
    return L


def lib():
    """The library, for launching work: additionally requires a visible GPU."""
    global _gpu_ok
    L = load()
    if not _gpu_ok:
        if not torch.cuda.is_available():
            raise HipBackendError("backend='hip' needs a ROCm GPU (torch.cuda.is_available() is False); "
                                  "there is no CPU fallback for this backend")
        _gpu_ok = True
    return L


_gpu_ok = False


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().ms_last_error_string().decode("utf-8", "replace")
        raise HipBackendError(f"{what or 'libmojosplat_hip'} failed (status {rc}): {msg}")


def ptr(t):
    return None if t is None else c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream(device=None):
    """hipStream_t of torch's current stream on `device` (what every ms_* call is launched on)."""
    if _raw_stream is not None:
        idx = device.index if isinstance(device, torch.device) else device
        return c_void_p(_raw_stream(torch.cuda.current_device() if idx is None else idx))
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


class on_device:
    """`with on_device(dev):` -- torch.cuda.device(dev) only when dev is not already current (the
    context manager costs several microseconds per frame otherwise)."""

    def __init__(self, dev):
        idx = dev.index if isinstance(dev, torch.device) else dev
        self.ctx = None if idx is None or idx == torch.cuda.current_device() else torch.cuda.device(idx)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def require_cuda(*tensors, what="input"):
    for t in tensors:
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError(f"backend='hip': every {what} must be a CUDA/ROCm tensor")


def f32c(t):
    """contiguous fp32 view/copy (no copy when already so)"""
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


# torch's own setter of version counters (what torch.autograd.graph's version-preserving context uses): one call for a list of
# tensors, ~0.3 us a tensor against ~5 us for an in-place op on an empty view.  Private to torch: where it is missing or takes
# other arguments, the in-place op does the same.
_set_versions = getattr(torch._C._autograd, "_unsafe_set_version_counter", None)


def bump(*tensors):
    """Move the version counter of every tensor a kernel has just written through its raw pointer -- nothing is launched,
    nothing is copied.  The package's caches (the band path's ms_scene, a prepared scene's bounds, a camera's centre) and
    autograd's saved-tensor check go by ``_version``; every ``backend="hip"`` entry point that writes a caller's tensor in
    place calls this where its ``backend="torch"`` definition moves the counter ("In-place writers")."""
    global _set_versions
    if _set_versions is not None:
        try:
            _set_versions(tensors, [t._version + 1 for t in tensors])
            return
        except Exception:                        # noqa: BLE001  (another torch: other arguments, or a setter that refuses)
            _set_versions = None                 # ... the in-place op below from now on: it moves every counter of this call too
    for t in tensors:
        t.detach().unsqueeze(0)[:0].zero_()     # (an empty view; unsqueeze: a 0-dim parameter has no rows to slice)


def config_depth_cut(mode=None, min_pairs=None):
    """Depth cut-offs of the fused frame (include/mojosplat_hip.h, ms_config_depth_cut): mode 0 never / 1 from
    `min_pairs` pairs on (the default: 6 M) / 2 on every frame that can.  Process-wide; None leaves a setting alone.
    The library reads MOJOSPLAT_DEPTH_CUT / MOJOSPLAT_DEPTH_CUT_MIN_PAIRS once -- tests and measurements that switch
    inside one process call this instead of writing os.environ."""
    check(lib().ms_config_depth_cut(-1 if mode is None else int(mode), -1 if min_pairs is None else int(min_pairs)),
          "ms_config_depth_cut")


def config_fused_sort(mode=None):
    """Sort + rasterise in one launch (include/mojosplat_hip.h, ms_config_fused_sort): mode 0 never / 1 where the
    rasteriser runs two waves a block by its own rule (the default) / 2 on every whole frame of plain 32-px bins.
    Adding 4 to mode 1 or 2 keeps the clean-up launch behind such a frame; without it the bins of a fused frame that
    has no depth cut finish their own short fronts in the kernel (bit 49 of the frame's flag word) and nothing follows it.
    Process-wide; None leaves it alone.  The library reads MOJOSPLAT_FUSED_SORT once -- tests and measurements that
    switch inside one process call this instead of writing os.environ."""
    check(lib().ms_config_fused_sort(-1 if mode is None else int(mode)), "ms_config_fused_sort")
