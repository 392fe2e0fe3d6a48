"""Shared scene builders for the test-suite (CPU generators -> identical bytes everywhere).

Scenes restate the fixtures of the reference's tests: tests/test_projection_mojo.py:16-46,
tests/test_rasterization.py:18-36.
"""
import glob
import os

import numpy as np
import torch

from mojosplat_amd import Camera

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


def load_golden(path):
    d = np.load(path)
    H, W = (int(v) for v in d["HW"])
    fx, fy, cx, cy = (float(v) for v in d["intr"])
    near, far = (float(v) for v in d["nearfar"])
    return d, dict(H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, near=near, far=far)


def camera_from_golden(d, cam, device="cpu"):
    vm = torch.from_numpy(d["viewmat"]).to(device)
    return Camera(R=vm[:3, :3].contiguous(), T=vm[:3, 3].contiguous(), H=cam["H"], W=cam["W"],
                  fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], near=cam["near"],
                  far=cam["far"])


def simple_camera(device="cpu", H=64, W=64, f=100.0, T=(0.0, 0.0, 0.0)):
    return Camera(R=torch.eye(3, device=device), T=torch.tensor(T, dtype=torch.float32, device=device),
                  H=H, W=W, fx=f, fy=f, cx=W / 2.0, cy=H / 2.0, near=0.1, far=100.0)


def proj_scene(N, seed=42, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    means3d = torch.randn(N, 3, generator=g) * 2.0
    means3d[:, 2] = means3d[:, 2].abs() + 1.0
    scales = torch.log(torch.rand(N, 3, generator=g) * 0.3 + 0.05)
    quats = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), p=2, dim=-1)
    opac = torch.sigmoid(torch.randn(N, generator=g))
    return [t.to(device) for t in (means3d, scales, quats, opac)]


def raster_scene(N, seed=0, device="cpu", depth_range=(1.5, 5.0), scale_log=-2.0,
                 opacity_range=(0.5, 0.95), channels=3):
    g = torch.Generator().manual_seed(seed)
    means3d = torch.randn(N, 3, generator=g)
    means3d[:, 2] = torch.rand(N, generator=g) * (depth_range[1] - depth_range[0]) + depth_range[0]
    ls = torch.ones(N, 3) * scale_log + torch.randn(N, 3, generator=g) * 0.1
    quats = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=1)
    opac = torch.rand(N, generator=g) * (opacity_range[1] - opacity_range[0]) + opacity_range[0]
    colors = torch.rand(N, channels, generator=g)
    return [t.to(device) for t in (means3d, ls, quats, opac, colors)]


def np_(t):
    return t.detach().cpu().numpy()


def oracle_project(oracle, means3d, scales, quats, opac, cam, **kw):
    vm = np_(cam.view_matrix)
    return oracle.project_fwd(np_(means3d), np_(scales), np_(quats), None if opac is None else np_(opac),
                              vm, cam.fx, cam.fy, cam.cx, cam.cy, cam.W, cam.H, near=cam.near,
                              far=cam.far, **kw)


# ------------------------------------------------------------------ the projection parity bar
def check_projection(hip_out, orc_out, max_flips=0):
    m2, con, dep, rad = (np_(t) for t in hip_out)
    om2, ocon, odep, orad = orc_out
    flips = np.nonzero((rad != orad).any(1))[0]
    assert len(flips) <= max_flips, f"{len(flips)} radius mismatches"
    if len(flips):
        # a flip is a +-1 px radius or a cull decision on the viewport edge
        both = (rad[flips] > 0).all(1) & (orad[flips] > 0).all(1)
        assert (np.abs(rad[flips][both] - orad[flips][both]) <= 1).all()
    ok = np.ones(len(rad), bool)
    ok[flips] = False
    np.testing.assert_allclose(m2[ok], om2[ok], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(dep[ok], odep[ok], rtol=1e-6, atol=1e-6)
    scale = np.abs(ocon[ok]).max(axis=1, keepdims=True) + 1e-30
    assert np.max(np.abs(con[ok] - ocon[ok]) / scale, initial=0.0) < 2e-5
    culled = ok & ~(orad > 0).all(1)
    assert (m2[culled] == 0).all() and (con[culled] == 0).all() and (dep[culled] == 0).all()
    return len(flips)


# ------------------------------------------------------------------ the raster parity bar
# North star: <= 1e-4 abs per pixel fp32 against the reference rasteriser
# (reference tests/test_rasterization.py:110: atol = rtol = 1e-4).  Two fp32 implementations of the
# compositor agree to rounding everywhere EXCEPT where one of its three data-dependent branches
# (alpha >= 1/255, T(1-alpha) <= 1e-4, sigma < 0) sits within rounding of its threshold: there one of
# them blends a Gaussian the other skips and the pixel moves by up to ~1/255.  The oracle reports, per
# pixel, how close any branch of its walk came to its threshold (`margin`, see orc_rasterize_fwd_rows);
# a pixel may exceed `atol` only if that margin is below `eps` -- zero unexplained pixels is asserted,
# and even explained ones are capped.  The counts go to stdout and gpurun_out/parity_counts.jsonl.
PARITY_LOG = os.path.join(os.path.dirname(GOLDEN_DIR), "..", "gpurun_out", "parity_counts.jsonl")


def check_image_strict(img, ref, margin, *, tag, atol=1e-4, eps=1e-5, flip_cap=1e-2, f64=None):
    """img, ref (H,W,C); margin (H,W) from the oracle.  f64: optional float64 oracle frame (its
    disagreement with the fp32 oracle is recorded beside the counts).  -> the record (dict)."""
    import json
    img = np_(img) if torch.is_tensor(img) else np.asarray(img)
    assert img.shape == ref.shape and np.isfinite(img).all()
    diff = np.abs(img.astype(np.float64) - ref.astype(np.float64)).max(axis=-1)
    bad = diff > atol
    sens = margin < eps
    rec = dict(tag=tag, pixels=int(diff.size), atol=atol, margin_eps=eps, beyond_atol=int(bad.sum()),
               explained_by_branch_margin=int((bad & sens).sum()), unexplained=int((bad & ~sens).sum()),
               branch_sensitive_pixels=int(sens.sum()), max_abs=float(diff.max()),
               max_abs_where_no_branch_is_close=float(diff[~sens].max()) if (~sens).any() else 0.0)
    if f64 is not None:
        d64 = np.abs(f64 - ref.astype(np.float64)).max(axis=-1)
        rec["oracle_f32_vs_f64_beyond_atol"] = int((d64 > atol).sum())
        rec["oracle_f32_vs_f64_beyond_atol_unexplained"] = int(((d64 > atol) & ~sens).sum())
    line = json.dumps(rec)
    print("PARITY", line)
    try:
        os.makedirs(os.path.dirname(PARITY_LOG), exist_ok=True)
        with open(PARITY_LOG, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass
    assert rec["unexplained"] == 0, f"{tag}: {rec['unexplained']} px beyond {atol} with no branch near its threshold: {rec}"
    assert rec["max_abs"] <= flip_cap, f"{tag}: max abs diff {rec['max_abs']:.3g}"
    return rec


# ------------------------------------------------------------------ gradient bars (round 5)
# Two bars per tensor.  (1) max norm: |g - g_ref| <= rel * max|g_ref| -- what rounds 1-4 asserted; it is blind to the error
# of the small-gradient majority.  (2) per element: every element with |g_ref| >= floor * max|g_ref| must agree to
# elem_rel RELATIVE to itself (and the 99.9th percentile of those errors to elem_p999).  The backward rasteriser's
# two-term bf16 tile (both terms rounded to nearest: 2^-18 per value) and its approximate reciprocal are what bar (2) watches.
# Where the bars sit (measured, profiles/r05_grad_stats.txt): against float64 autograd the worst element of any test is
# 3.4e-4 off -> 2e-3 on EVERY element.  Fused against the per-stage functions BOTH sides are fp32 with different orders of
# summation (the per-stage kernel walks back to front and recovers T by division): regular scenes up to 3e-3 on a single
# element of ~7 000 (a sum that nearly cancels), 99.9 % within 5e-4 -> 5e-3 on every element, 1e-3 on the 99.9th
# percentile; the adversarial stacks (thousands of faint entries at one depth behind every pixel) 1.6e-2 / 2.3e-3 ->
# 5e-2 / 5e-3.
def grad_stats(got, ref, floor=1e-3):
    """-> dict(scale, max_norm_err, checked, elem_rel_max, elem_rel_p999, worst_index): got / ref arrays or tensors."""
    got = (np_(got) if torch.is_tensor(got) else np.asarray(got)).astype(np.float64).reshape(-1)
    ref = (np_(ref) if torch.is_tensor(ref) else np.asarray(ref)).astype(np.float64).reshape(-1)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    err = np.abs(got - ref)
    out = dict(scale=scale, max_norm_err=float(err.max() / scale) if scale > 0 else 0.0, checked=0, elem_rel_max=0.0,
               elem_rel_p999=0.0, worst_index=-1)
    if scale > 0:
        sel = np.abs(ref) >= floor * scale
        if sel.any():
            rel = err[sel] / np.abs(ref[sel])
            out.update(checked=int(sel.sum()), elem_rel_max=float(rel.max()), elem_rel_p999=float(np.quantile(rel, 0.999)),
                       worst_index=int(np.flatnonzero(sel)[int(rel.argmax())]))
    return out


GRAD_LOG = os.path.join(os.path.dirname(GOLDEN_DIR), "..", "gpurun_out", "grad_stats.jsonl")


def assert_grad_close(name, got, ref, rel=2e-3, elem_rel=None, floor=1e-3, elem_p999=None):
    """GRAD_BARS_SOFT=1 in the environment records the per-element statistics (gpurun_out/grad_stats.jsonl) without
    asserting them -- for calibrating the bars; the max-norm bar is always asserted."""
    import inspect
    import json
    st = grad_stats(got, ref, floor)
    try:
        os.makedirs(os.path.dirname(GRAD_LOG), exist_ok=True)
        with open(GRAD_LOG, "a") as f:
            f.write(json.dumps(dict(test=os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], name=name, rel=rel,
                                    elem_rel=elem_rel, **st)) + "\n")
    except OSError:
        pass
    assert st["max_norm_err"] * st["scale"] <= rel * st["scale"] + 1e-6, f"{name}: max-norm bar {rel}: {st}"
    if os.environ.get("GRAD_BARS_SOFT") != "1":
        if elem_rel is not None:
            assert st["elem_rel_max"] <= elem_rel, f"{name}: per-element bar {elem_rel} (|g_ref| >= {floor} max): {st}"
        if elem_p999 is not None:
            assert st["elem_rel_p999"] <= elem_p999, f"{name}: 99.9th percentile of the per-element error > {elem_p999}: {st}"
    return st


# ------------------------------------------------------------------ general pinhole cameras
# fx != fy and an off-centre principal point: the FOV clamp's two sides differ (lim_pos != lim_neg) and any fx / fy swap
# changes the numbers.  Scenes are placed in CAMERA space -- in view, past each of the four clamp limits with an extent
# that still reaches the image (alive, clamped Jacobian), at the near / far planes, and culled -- then mapped to world.
SIDES = ("x_pos", "x_neg", "y_pos", "y_neg")
KINK = 1e-4     # a Gaussian within this of a limit (in x/z or y/z) sits on the clamp's kink: none is placed there


def fov_limits(cam):
    """The clamp limits on x/z and y/z (csrc/project_device.hpp make_proj_params, oracle/torch_oracle.py), float64."""
    tx, ty = 0.5 * cam.W / cam.fx, 0.5 * cam.H / cam.fy
    return dict(x_pos=(cam.W - cam.cx) / cam.fx + 0.3 * tx, x_neg=cam.cx / cam.fx + 0.3 * tx,
                y_pos=(cam.H - cam.cy) / cam.fy + 0.3 * ty, y_neg=cam.cy / cam.fy + 0.3 * ty)


def general_camera(W, H, fx, fy, cx, cy, *, near=0.5, far=30.0, eye=(1.8, -1.2, -4.5), target=(0.3, 0.2, 0.4),
                   device="cpu"):
    from mojosplat_amd.utils import look_at
    vm = look_at(torch.tensor(eye), torch.tensor(target), torch.tensor([0.0, 1.0, 0.0]))
    return Camera(R=vm[:3, :3].contiguous().to(device), T=vm[:3, 3].contiguous().to(device), H=H, W=W, fx=fx, fy=fy,
                  cx=cx, cy=cy, near=near, far=far)


def _posed(cam):
    """The same camera with a view matrix of its own that requires grad (the camera pose as a leaf)."""
    vm = cam.view_matrix.detach().clone().requires_grad_(True)
    return Camera(R=cam.R, T=cam.T, H=cam.H, W=cam.W, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, near=cam.near,
                  far=cam.far, view_matrix=vm)


# name -> (W, H, fx, fy, cx, cy, near, far, axes whose principal point is off-centre)
GENERAL_CAMERAS = {
    "fx>fy_pp_xy": (330, 190, 300.0, 240.0, 0.35 * 330, 0.62 * 190, 0.5, 30.0, "xy"),
    "fy>fx_pp_x": (330, 190, 240.0, 300.0, 0.68 * 330, 95.0, 0.5, 30.0, "x"),
    "fx>fy_pp_y": (330, 190, 280.0, 224.0, 165.0, 0.3 * 190, 0.5, 30.0, "y"),
    "fy>fx_pp_xy": (330, 190, 230.0, 287.5, 0.7 * 330, 0.33 * 190, 0.5, 30.0, "xy"),
    "crop_cx<0": (330, 190, 300.0, 240.0, -0.25 * 330, 0.7 * 190, 0.5, 30.0, "xy"),
    "crop_cy>H": (330, 190, 240.0, 300.0, 0.3 * 330, 1.3 * 190, 0.5, 30.0, "xy"),
    "near2_far7": (330, 190, 300.0, 240.0, 0.38 * 330, 0.67 * 190, 2.0, 7.0, "xy"),
}


def camera_by_name(name, device="cpu", **kw):
    W, H, fx, fy, cx, cy, near, far, _ = GENERAL_CAMERAS[name]
    return general_camera(W, H, fx, fy, cx, cy, near=near, far=far, device=device, **kw)


def assert_general_camera(cam, axes="xy"):
    """The camera is not the centred, square one: |fx/fy - 1| >= 0.2 and, on every axis in `axes`, the two clamp limits
    differ by at least 30 % of the larger one."""
    assert abs(cam.fx / cam.fy - 1.0) >= 0.2 - 1e-9, (cam.fx, cam.fy)
    L = fov_limits(cam)
    for a in axes:
        p, n = L[a + "_pos"], L[a + "_neg"]
        assert abs(p - n) >= 0.3 * max(abs(p), abs(n)), (a, p, n)


def general_scene(cam, *, n_view=1200, n_side=40, n_plane=24, n_cull=24, seed=0, channels=3, z_range=None,
                  view_scale=(0.015, 0.1)):
    """-> dict(means3d, scales, quats, opacities, features) (float32, CPU) and `kind` (N,) int: 0 in view, 1..4 past
    SIDES[k - 1], 5 at the near / far plane, 6 culled (behind the camera, far off-screen, opacity < 1/255).
    A side Gaussian sits 0.01 .. 0.1 past its limit (its centre 0.15 W + fx d beyond the image's edge) and is isotropic
    with a footprint 1.1 .. 1.7 times that distance: its extent reaches into the image.  z_range (in-view depths):
    default 2.5 .. 8, or half the near plane .. 1.3 x the far plane when near >= 1 (the planes cut through the scene)."""
    if z_range is None:
        z_range = (2.5, 8.0) if cam.near < 1.0 else (0.5 * cam.near, 1.3 * cam.far)
    g = torch.Generator().manual_seed(seed)
    rnd = lambda n, lo, hi: torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo
    W, H, fx, fy, cx, cy = cam.W, cam.H, cam.fx, cam.fy, cam.cx, cam.cy
    L = fov_limits(cam)
    parts, kinds, sc, op = [], [], [], []

    def add(u, v, z, s, o, k):
        parts.append(torch.stack([u * z, v * z, z], -1))
        sc.append(s)
        op.append(o)
        kinds.append(torch.full((len(z),), k, dtype=torch.int64))

    # in view: centres over the image and a margin of 0.1 W / 0.1 H (the limits sit 0.15 W / H out)
    z = rnd(n_view, *z_range)
    add((rnd(n_view, -0.1 * W, 1.1 * W) - cx) / fx, (rnd(n_view, -0.1 * H, 1.1 * H) - cy) / fy, z,
        torch.exp(rnd(n_view, np.log(view_scale[0]), np.log(view_scale[1]))), rnd(n_view, 0.2, 0.95), 0)
    # past each limit
    for k, side in enumerate(SIDES):
        d = rnd(n_side, 0.01, 0.1)
        z = rnd(n_side, 2.5, 6.0)
        o = rnd(n_side, 0.3, 0.8)
        ext = torch.sqrt(2.0 * torch.log(255.0 * o))
        if side[0] == "x":
            f, span, lim = fx, W, L[side]
            u = lim + d if side == "x_pos" else -lim - d
            v = (rnd(n_side, 0.1 * H, 0.9 * H) - cy) / fy
        else:
            f, span, lim = fy, H, L[side]
            v = lim + d if side == "y_pos" else -lim - d
            u = (rnd(n_side, 0.1 * W, 0.9 * W) - cx) / fx
        dist = 0.15 * span + f * d
        s = rnd(n_side, 1.1, 1.7) * dist * z / (ext * f * np.sqrt(1.0 + lim * lim))
        add(u, v, z, s, o, 1 + k)
    # at the planes: just in front of / behind the near plane and the far plane
    h = n_plane // 2
    zn = cam.near * torch.cat([rnd(h // 2, 0.9, 0.99), rnd(h - h // 2, 1.01, 1.1)])
    zf = cam.far * torch.cat([rnd(h // 2, 0.98, 0.999), rnd(h - h // 2, 1.001, 1.02)])
    z = torch.cat([zn, zf])
    sig = rnd(n_plane, 1.5, 4.0)   # px
    add((rnd(n_plane, 0.1 * W, 0.9 * W) - cx) / fx, (rnd(n_plane, 0.1 * H, 0.9 * H) - cy) / fy, z, sig * z / fx,
        rnd(n_plane, 0.4, 0.9), 5)
    # culled: behind the camera, far off-screen, nearly transparent
    c3 = n_cull // 3
    z = rnd(n_cull, 2.5, 6.0)
    z[:c3] = -z[:c3]
    u = (rnd(n_cull, 0.2 * W, 0.8 * W) - cx) / fx
    u[c3:2 * c3] = 4.0 * (L["x_pos"] + 1.0)
    o = rnd(n_cull, 0.3, 0.9)
    o[2 * c3:] = 0.002
    add(u, (rnd(n_cull, 0.2 * H, 0.8 * H) - cy) / fy, z, rnd(n_cull, 0.03, 0.08), o, 6)

    pc = torch.cat(parts)
    N = pc.shape[0]
    R, t = cam.R.detach().cpu().double(), cam.T.detach().cpu().double()
    means3d = ((pc - t) @ R).float().contiguous()
    s = torch.cat(sc)
    kind = torch.cat(kinds)
    iso = (kind >= 1) & (kind <= 4)
    scales = torch.log(s)[:, None].repeat(1, 3) + torch.where(iso[:, None], 0.0, 0.3 * torch.randn(N, 3, generator=g, dtype=torch.float64))
    quats = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=1)
    scene = dict(means3d=means3d, scales=scales.float().contiguous(), quats=quats.contiguous(),
                 opacities=torch.cat(op).float().contiguous(), features=torch.rand(N, channels, generator=g).contiguous())
    return scene, kind


def clamp_counts(means3d, cam, alive):
    """Alive Gaussians whose x/z or y/z lies beyond each limit by more than KINK (float64) -> dict side -> count, and
    the mask of Gaussians within KINK of any limit."""
    m = torch.as_tensor(np.asarray(np_(means3d) if torch.is_tensor(means3d) else means3d), dtype=torch.float64)
    vm = cam.view_matrix.detach().cpu().double()
    pc = m @ vm[:3, :3].T + vm[:3, 3]
    u, v = (pc[:, 0] / pc[:, 2]).numpy(), (pc[:, 1] / pc[:, 2]).numpy()
    L = fov_limits(cam)
    alive = np.asarray(np_(alive) if torch.is_tensor(alive) else alive, bool)
    past = dict(x_pos=u > L["x_pos"] + KINK, x_neg=u < -L["x_neg"] - KINK, y_pos=v > L["y_pos"] + KINK,
                y_neg=v < -L["y_neg"] - KINK)
    kink = (np.abs(u - L["x_pos"]) <= KINK) | (np.abs(u + L["x_neg"]) <= KINK) | (np.abs(v - L["y_pos"]) <= KINK) | \
        (np.abs(v + L["y_neg"]) <= KINK)
    return {k: int((alive & p).sum()) for k, p in past.items()}, kink
