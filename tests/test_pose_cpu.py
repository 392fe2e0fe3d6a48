"""CPU: the pose-gradient surface that needs no GPU -- the C ABI's new entry points validate their output and scratch
before touching the device, and the sharded trainer refuses a camera pose that requires grad."""
import ctypes

import pytest
import torch

from helpers import simple_camera
from mojosplat_amd import Camera, _hip

OK, INVALID, WORKSPACE = 0, 1, 2


def _lib():
    import os
    if not os.path.exists(_hip.library_path()):
        from mojosplat_amd.csrc import build
        build.build()
    return _hip.load()


def test_pose_scratch_bytes():
    L = _lib()
    assert L.ms_pose_scratch_bytes(0) >= 64
    assert L.ms_pose_scratch_bytes(256) >= 64 and L.ms_pose_scratch_bytes(257) >= 128
    assert L.ms_pose_scratch_bytes(1 << 20) >= (1 << 20) // 256 * 64
    assert all(L.ms_pose_scratch_bytes(n) % 256 == 0 for n in (1, 255, 256, 10000))


def test_pose_entry_points_validate_scratch():
    L = _lib()
    P = ctypes.c_void_p(0x1000)
    N = ctypes.c_int64(1000)
    need = L.ms_pose_scratch_bytes(1000)
    err = lambda: L.ms_last_error_string().decode()
    args = (N, P, P, 1, P, P, 100., 100., 32., 32., 64, 64, .3, P, P, P, None, P, P, P)
    assert L.ms_project_gaussians_bwd_pose(*args, P, P, need - 1, None) == WORKSPACE and "pose scratch" in err()
    assert L.ms_project_gaussians_bwd_pose(*args, P, None, need, None) == INVALID and "scratch" in err()
    assert L.ms_project_gaussians_bwd_pose(*args, ctypes.c_void_p(0x1002), P, need, None) == INVALID and "aligned" in err()
    fin = (N, P, P, 1, P, P, 3, P, 100., 100., 32., 32., 64, 64, .3, P, P, P, P, P, P)
    assert L.ms_render_bwd_finish_pose(*fin, P, P, need - 1, None) == WORKSPACE
    assert L.ms_render_bwd_finish_densify_pose(*fin, .1, 100., P, P, P, P, P, 16, None) == WORKSPACE
    sh = (N, 16, 3, P, 0., 0., 0., P, None, 1, P, P, P, P)
    assert L.ms_spherical_harmonics_bwd_pose(*sh, P, P, 64, None) == WORKSPACE
    assert L.ms_spherical_harmonics_bwd_pose(N, 16, 3, P, 0., 0., 0., None, None, 1, P, P, None, None, P, P, need,
                                             None) == INVALID and "coefficients" in err()
    # a NULL pose output: the namesake's own checks, nothing more (a bad camera is still refused first)
    assert L.ms_project_gaussians_bwd_pose(N, P, P, 1, P, P, 0., 100., 32., 32., 64, 64, .3, P, P, P, None, P, P, P,
                                           None, None, 0, None) == INVALID and "camera" in err()


def test_sharded_trainer_refuses_a_pose_that_requires_grad():
    from mojosplat_amd.distributed import render_gaussians_trainable_sharded
    cam = simple_camera()
    vm = cam.view_matrix.clone().requires_grad_(True)
    pcam = Camera(R=cam.R, T=cam.T, H=cam.H, W=cam.W, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, view_matrix=vm)
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="camera pose"):
        render_gaussians_trainable_sharded(z, z, torch.zeros(4, 4), torch.zeros(4), z, pcam)
