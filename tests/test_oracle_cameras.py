"""CPU: the C oracle (oracle/gsplat_oracle.c) against the float64 restatement (oracle/torch_oracle.py) at general pinhole
cameras -- fx != fy, the principal point toward each corner and outside the image -- with Gaussians in the FOV clamp's
regime past each of its four limits.  Every GPU test of tests/test_hip_cameras.py compares against this oracle; the
golden fixtures pin it to the reference only at one such camera (general_cam_n800_250x170)."""
import numpy as np
import pytest
import torch

import oracle
from helpers import (GENERAL_CAMERAS, SIDES, assert_general_camera, camera_by_name, check_image_strict, clamp_counts,
                     general_scene, np_, oracle_project)
from oracle import torch_oracle

MIN_CLAMPED = 20    # alive Gaussians past each limit, per camera (40 are placed)


def _f64(a):
    return torch.from_numpy(np.asarray(a)).double()


def _radii_f64(con, op):
    """gsplat's opacity-aware per-axis radius from float64 conics: ceil(min(3.33, sqrt(2 ln(255 o))) sqrt(cov_axis))."""
    a, b, c = con[:, 0], con[:, 1], con[:, 2]
    det = a * c - b * b
    ext = np.minimum(3.33, np.sqrt(2.0 * np.log(np.maximum(255.0 * op, 1.0))))
    return np.stack([np.ceil(ext * np.sqrt(c / det)), np.ceil(ext * np.sqrt(a / det))], -1)


@pytest.mark.parametrize("name", list(GENERAL_CAMERAS))
def test_oracle_projection_vs_float64_at_general_cameras(name):
    cam = camera_by_name(name)
    assert_general_camera(cam, GENERAL_CAMERAS[name][-1])
    sc, kind = general_scene(cam, seed=3)
    m2, con, dep, rad = oracle_project(oracle, sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], cam)
    alive = (rad > 0).all(1)
    counts, kink = clamp_counts(sc["means3d"], cam, alive)
    print(name, "alive", int(alive.sum()), "clamped", counts)
    assert not kink.any()
    assert all(counts[s] >= MIN_CLAMPED for s in SIDES), counts
    k = kind.numpy()
    assert not alive[k == 6].any(), "behind the camera / off-screen / transparent: culled"
    near_far = k == 5
    z = (np_(sc["means3d"]).astype(np.float64) @ np_(cam.R).T.astype(np.float64) + np_(cam.T))[:, 2]
    assert (alive[near_far] == ((z[near_far] >= cam.near) & (z[near_far] <= cam.far))).all(), "near / far planes"
    rm2, rcon, rdep = torch_oracle.project(_f64(sc["means3d"]), _f64(sc["scales"]), _f64(sc["quats"]),
                                           cam.view_matrix.double(), cam.fx, cam.fy, cam.cx, cam.cy, cam.W, cam.H)
    rm2, rcon, rdep = rm2.numpy()[alive], rcon.numpy()[alive], rdep.numpy()[alive]
    np.testing.assert_allclose(m2[alive], rm2, rtol=1e-6, atol=2e-4)
    np.testing.assert_allclose(dep[alive], rdep, rtol=1e-6)
    scale = np.abs(rcon).max(axis=1, keepdims=True)
    assert np.max(np.abs(con[alive] - rcon) / scale) < 2e-5
    rr = _radii_f64(rcon, np_(sc["opacities"]).astype(np.float64)[alive])
    off = np.abs(rad[alive] - rr)
    assert off.max() <= 1 and (off > 0).sum() <= 2, "radii: the clamped Jacobian's extent"


@pytest.mark.parametrize("name", ["fx>fy_pp_xy", "fy>fx_pp_xy", "crop_cx<0", "crop_cy>H", "near2_far7"])
def test_oracle_render_vs_float64_at_general_cameras(name):
    cam = camera_by_name(name)
    sc, _ = general_scene(cam, seed=4)
    cpu = {k: np_(v) for k, v in sc.items()}
    bg = np.array([0.2, 0.1, 0.3], np.float32)
    img, aux = oracle.render_fwd(cpu["means3d"], cpu["scales"], cpu["quats"], cpu["opacities"], cpu["features"],
                                 np_(cam.view_matrix), cam.fx, cam.fy, cam.cx, cam.cy, cam.W, cam.H, background=bg,
                                 near=cam.near, far=cam.far, margin=True)
    counts, _ = clamp_counts(sc["means3d"], cam, (aux["radii"] > 0).all(1))
    assert all(counts[s] >= MIN_CLAMPED for s in SIDES), counts
    ref, _ = torch_oracle.rasterize(_f64(aux["means2d"]), _f64(aux["conics"]), _f64(cpu["features"]), _f64(cpu["opacities"]),
                                    _f64(bg), torch.from_numpy(aux["ranges"]), torch.from_numpy(aux["ids"]), cam.H, cam.W, 16)
    rec = check_image_strict(img, ref.numpy(), aux["margin"], tag=f"oracle vs float64 at {name}", eps=2e-5)
    assert rec["max_abs_where_no_branch_is_close"] <= 1e-4
