"""GPU: every HIP path at general pinhole cameras -- fx != fy (ratio 1.25 and 0.8), the principal point off-centre in x,
in y and in both, outside the image (crop-style), near / far planes that cut through the scene, ragged 330 x 190 frames.

At the centred, square camera the rest of the suite uses, an fx / fy swap or a swap of the FOV clamp's two sides
(lim_pos / lim_neg, cx / W - cx) changes no number; these formulas are written out separately in the projection
(make_proj_params), the three backward parameter set-ups of csrc/project_bwd.hip, the band pre-cull (csrc/binning.hip) and
the batch's per-view intrinsics (csrc/pipeline.hip).  Scenes come from tests/helpers.py general_scene: Gaussians in view,
alive Gaussians past each of the four clamp limits (a clamped Jacobian), at the near / far planes, and culled ones.

Every test asserts its regime: the camera is general (helpers.assert_general_camera: |fx/fy - 1| >= 0.2, the limits of an
off-centre axis 30 % apart) and a minimum of alive, clamped Gaussians per side (float64, none within 1e-4 of a limit).
Bars are the suite's: check_projection (test_hip_parity.py), check_image_strict against oracle.render_fwd, bit equality
between paths that must agree, and test_hip_backward_paths.py's float64 autograd bars and branch guard for gradients."""
import math

import numpy as np
import pytest
import torch

import mojosplat_amd as ms
import oracle
from helpers import (GENERAL_CAMERAS, SIDES, assert_general_camera, assert_grad_close, camera_by_name, check_image_strict,
                     check_projection, clamp_counts, general_camera, general_scene, np_, oracle_project)
from mojosplat_amd import _fused
from mojosplat_amd import _hip as _hip_mod
from mojosplat_amd.autograd import project_gaussians_autograd, render_gaussians_trainable
from mojosplat_amd.binning import bin_gaussians_to_tiles_hip
from mojosplat_amd.densify import DensifyStats, update_torch
from mojosplat_amd.utils import Camera
from oracle import torch_oracle
from test_hip_backward_paths import ELEM_F64, Upstream
from test_hip_densify import F64_2D

pytestmark = pytest.mark.gpu

MIN_CLAMPED = 20                     # alive Gaussians past each limit (40 are placed per side)
NAMES = ("means3d", "scales", "quats", "opacities", "features")
BG = (0.2, 0.1, 0.3)


@pytest.fixture(autouse=True)
def _default_depth_cut_after_each_test():
    """Some tests force the depth cut (ms_config_depth_cut); every test leaves the library's default behind."""
    yield
    _hip_mod.config_depth_cut(1, 6_000_000)


def _scene(name, device, seed=0, **kw):
    cam = camera_by_name(name, device)
    assert_general_camera(cam, GENERAL_CAMERAS[name][-1])
    sc, kind = general_scene(cam, seed=seed, **kw)
    return {k: v.to(device) for k, v in sc.items()}, kind, cam


def _assert_clamped(sc, cam, radii, tag):
    counts, kink = clamp_counts(sc["means3d"], cam, (np.asarray(np_(radii) if torch.is_tensor(radii) else radii) > 0).all(1))
    print("REGIME", tag, "clamped per side", counts)
    assert not kink.any(), f"{tag}: a Gaussian on the clamp's kink"
    assert all(counts[s] >= MIN_CLAMPED for s in SIDES), f"{tag}: {counts}"


def _oracle_frame(sc, cam, bg, tile_size=16, feats=None):
    cpu = {k: np_(v) for k, v in sc.items()}
    f = cpu["features"] if feats is None else feats
    return oracle.render_fwd(cpu["means3d"], cpu["scales"], cpu["quats"], cpu["opacities"], f.astype(np.float32),
                             np_(cam.view_matrix), cam.fx, cam.fy, cam.cx, cam.cy, cam.W, cam.H, background=np.asarray(bg, np.float32),
                             tile_size=tile_size, near=cam.near, far=cam.far, margin=True, threads=8)


def _stagewise(sc, cam, bg, tile_size=16):
    m2, con, dep, rad = ms.project_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], cam, backend="hip")
    ids, ranges = ms.bin_gaussians_to_tiles(m2, rad, dep, cam.H, cam.W, tile_size, backend="hip")
    if ids.numel() == 0:
        return torch.zeros(cam.H, cam.W, sc["features"].shape[1], device=m2.device)
    return ms.rasterize_gaussians(m2, con, sc["features"], sc["opacities"], bg, ranges, ids, cam, tile_size=tile_size,
                                  backend="hip")


def _args(sc):
    return tuple(sc[k] for k in NAMES)


# ------------------------------------------------------------------ a. projection forward
@pytest.mark.parametrize("name", list(GENERAL_CAMERAS))
def test_projection_at_general_cameras(device, name):
    """project_gaussians(backend="hip") against the C oracle (check_projection's bar) and, on the alive rows, means2d and
    conics against float64 torch_oracle.project.  The near / far Gaussians are culled exactly by the planes."""
    sc, kind, cam = _scene(name, device, seed=10)
    out = ms.project_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], cam, backend="hip")
    cpu = {k: v.cpu() for k, v in sc.items()}
    ref = oracle_project(oracle, cpu["means3d"], cpu["scales"], cpu["quats"], cpu["opacities"], cam)
    check_projection(out, ref, max_flips=1)
    m2, con, dep, rad = (np_(t) for t in out)
    alive = (rad > 0).all(1)
    _assert_clamped(sc, cam, rad, name)
    k = kind.numpy()
    assert not alive[k == 6].any()
    z = (cpu["means3d"].double() @ cam.R.cpu().double().T + cam.T.cpu().double())[:, 2].numpy()
    nf = k == 5
    assert (alive[nf] == ((z[nf] >= cam.near) & (z[nf] <= cam.far))).all()
    assert alive[nf].any() and not alive[nf].all()
    f64 = lambda t: t.double()
    rm2, rcon, _ = torch_oracle.project(f64(cpu["means3d"]), f64(cpu["scales"]), f64(cpu["quats"]), cam.view_matrix.cpu().double(),
                                        cam.fx, cam.fy, cam.cx, cam.cy, cam.W, cam.H)
    rm2, rcon = rm2.numpy()[alive], rcon.numpy()[alive]
    np.testing.assert_allclose(m2[alive], rm2, rtol=1e-6, atol=2e-4)
    scale = np.abs(rcon).max(axis=1, keepdims=True)
    assert np.max(np.abs(con[alive] - rcon) / scale) < 2e-5


# ------------------------------------------------------------------ b. the fused forward frame
FRAME_CASES = [("ts16_bin16", 16, 16), ("ts16_bin32", 16, 32), ("ts16_bin64", 16, 64), ("ts8", 8, None),
               ("ts24", 24, None), ("ts32", 32, None), ("fp16", 16, None), ("per_stage", 16, None)]


@pytest.mark.parametrize("name", ["fx>fy_pp_xy", "fy>fx_pp_xy", "crop_cx<0", "crop_cy>H", "near2_far7"])
def test_forward_frames_at_general_cameras(device, name):
    """render_gaussians on the default path at tile size 16 with bins of 16 / 32 / 64 px, at tile sizes 8 / 24 / 32, with
    fp16 features, and the per-stage path: each against oracle.render_fwd under check_image_strict."""
    sc, _, cam = _scene(name, device, seed=20)
    bg = torch.tensor(BG, device=device)
    for tag, ts, px in FRAME_CASES:
        if tag == "fp16":
            s16 = dict(sc, features=sc["features"].half())
            img = ms.render_gaussians(*_args(s16), cam, background_color=bg.half(), tile_size=ts)
            ref, aux = _oracle_frame(sc, cam, np_(bg.half().float()), ts, feats=np_(s16["features"].float()))
        elif tag == "per_stage":
            img = _stagewise(sc, cam, bg, ts)
            ref, aux = _oracle_frame(sc, cam, BG, ts)
        else:
            img = ms.render_gaussians(*_args(sc), cam, background_color=bg, tile_size=ts, bin_size=px)
            ref, aux = _oracle_frame(sc, cam, BG, ts)
        if tag in ("ts16_bin16", "ts8"):
            _assert_clamped(sc, cam, aux["radii"], f"{name}/{tag}")
        check_image_strict(img.float(), ref, aux["margin"], tag=f"cameras/{name}/{tag}", eps=2e-5)


# ------------------------------------------------------------------ c. the multi-view batch
def _batch_cams(device):
    """Four views that share W, H, near and far and differ in fx, fy, cx, cy (and the pose)."""
    intr = [(300.0, 240.0, 0.35 * 330, 0.62 * 190), (230.0, 287.5, 0.7 * 330, 0.33 * 190),
            (320.0, 250.0, -0.2 * 330, 0.7 * 190), (250.0, 320.0, 0.3 * 330, 1.25 * 190)]
    eyes = [(1.8, -1.2, -4.5), (1.5, -1.0, -4.8), (2.0, -1.4, -4.2), (1.6, -1.1, -4.6)]
    return [general_camera(330, 190, *k, near=0.5, far=30.0, eye=e, device=device) for k, e in zip(intr, eyes)]


def test_multi_view_batch_with_per_view_intrinsics(device):
    """render_gaussians_batch over views with different intrinsics: each view bit-equal to render_gaussians for its
    camera and within check_image_strict of the oracle; the same views in reverse order give the same frames."""
    cams = _batch_cams(device)
    for c in cams:
        assert_general_camera(c)
    sc, _ = general_scene(cams[0], seed=30)
    sc = {k: v.to(device) for k, v in sc.items()}
    bg = torch.tensor(BG, device=device)
    singles = [ms.render_gaussians(*_args(sc), c, background_color=bg) for c in cams]
    batch = ms.render_gaussians_batch(*_args(sc), cams, background_color=bg)
    rev = ms.render_gaussians_batch(*_args(sc), cams[::-1], background_color=bg)
    for k, c in enumerate(cams):
        assert torch.equal(batch[k], singles[k]), f"view {k}"
        assert torch.equal(rev[len(cams) - 1 - k], singles[k]), f"reversed, view {k}"
        ref, aux = _oracle_frame(sc, c, BG)
        check_image_strict(batch[k], ref, aux["margin"], tag=f"cameras/batch/view{k}", eps=2e-5)
    for a in range(len(cams)):
        for b in range(a + 1, len(cams)):
            assert not torch.equal(singles[a], singles[b])


# ------------------------------------------------------------------ d. bands and the pre-cull
def _band_scene(cam, device, N=44_000, seed=40):
    """A plain scene of N Gaussians: general_scene's, many small in-view ones, and isotropic Gaussians centred just
    outside each 16-px row boundary whose y extent reaches 12 % of their radius into the next rows (the pre-cull's ry
    bound: with fx in place of fy it falls short of them when fy > fx)."""
    base, _ = general_scene(cam, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    rnd = lambda n, lo, hi: torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo
    edges = torch.arange(16, cam.H, 16, dtype=torch.float64)
    n_edge = 16 * len(edges)
    y_b = edges.repeat_interleave(16)
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(n_edge // 2)
    z = rnd(n_edge, 3.0, 6.0)
    o = rnd(n_edge, 0.7, 0.95)
    ext = torch.sqrt(2.0 * torch.log(255.0 * o))
    sig_y = rnd(n_edge, 15.0, 20.0)
    ry = torch.ceil(ext * sig_y)
    ys = y_b - sign * 0.88 * ry                          # above the boundary reaching down, below reaching up
    xs = rnd(n_edge, 0.2 * cam.W, 0.8 * cam.W)
    v = (ys - cam.cy) / cam.fy
    s = sig_y * z / (cam.fy * torch.sqrt(1.0 + v * v))
    pc = torch.stack([(xs - cam.cx) / cam.fx * z, v * z, z], -1)
    n_small = N - n_edge - base["means3d"].shape[0]
    zs = rnd(n_small, 2.5, 9.0)
    pcs = torch.stack([(rnd(n_small, -0.05 * cam.W, 1.05 * cam.W) - cam.cx) / cam.fx * zs,
                       (rnd(n_small, -0.05 * cam.H, 1.05 * cam.H) - cam.cy) / cam.fy * zs, zs], -1)
    R, t = cam.R.cpu().double(), cam.T.cpu().double()
    extra = dict(means3d=((torch.cat([pc, pcs]) - t) @ R).float(),
                 scales=torch.cat([torch.log(s)[:, None].repeat(1, 3), math.log(0.012) + 0.4 * torch.randn(n_small, 3, generator=g,
                                                                                                           dtype=torch.float64)]).float(),
                 quats=torch.nn.functional.normalize(torch.randn(n_edge + n_small, 4, generator=g), dim=1),
                 opacities=torch.cat([o, rnd(n_small, 0.2, 0.9)]).float(),
                 features=torch.rand(n_edge + n_small, 3, generator=g))
    sc = {k: torch.cat([base[k], extra[k]]).contiguous().to(device) for k in NAMES}
    return sc, n_edge


def test_band_frames_and_the_pre_cull_at_a_general_camera(device):
    """render_gaussians_sharded(..., rehearse=(r, world)) at worlds 3 and 8, on a camera with fy > fx and cy off-centre:
    a plain scene of 44k Gaussians (its bands are pre-culled) and the same scene through prepare_scene (the block bounds),
    with Gaussians just outside every row boundary that reach across it.  The assembled frame equals the single-GPU frame
    bit for bit; every band reports the pre-cull (flag bit 11) and fewer candidates than the frame has on its grid; one pass
    runs with the depth cut forced (three frames per band, each equal to the single-GPU frame's rows)."""
    from mojosplat_amd.distributed import render_gaussians_sharded
    from mojosplat_amd.scene_order import prepare_scene
    cam = camera_by_name("fy>fx_pp_xy", device)
    assert cam.fy > cam.fx and abs(cam.cy - cam.H / 2) > 0.1 * cam.H
    sc, n_edge = _band_scene(cam, device)
    bg = torch.tensor(BG, device=device)
    th = -(-cam.H // 16)
    ps = prepare_scene(*_args(sc))
    scenes = {"plain": _args(sc), "prepared": ps.arrays}
    regime = {}
    for label, g in scenes.items():
        ref = ms.render_gaussians(*g, cam, background_color=bg)
        full = {}
        _fused.render_fwd_hip(*g, cam, bg, 16, info=full)
        for world in (3, 8):
            rows = -(-th // world)
            for cut in (False, True):
                if cut and (label != "plain" or world != 8):
                    continue
                _hip_mod.config_depth_cut(2 if cut else 1, 6_000_000)
                _fused._state.clear()
                frame = torch.full_like(ref, -1.0)
                for r in range(world):
                    y0, y1 = min(r * rows * 16, cam.H), min((r + 1) * rows * 16, cam.H)
                    for _ in range(3 if cut else 1):
                        band = render_gaussians_sharded(*g, cam, background_color=bg, rehearse=(r, world))
                        assert torch.equal(band[y0:y1], ref[y0:y1]), (label, world, r, cut)
                    frame[y0:y1] = band[y0:y1]
                assert torch.equal(frame, ref), f"{label}: world {world}, cut {cut}"
            # the pre-cull ran on every non-empty band and dropped candidates
            _hip_mod.config_depth_cut(1, 6_000_000)
            for r in range(world):
                r0, r1 = min(r * rows, th), min((r + 1) * rows, th)
                if r1 <= r0:
                    continue
                info = {}
                buf = torch.zeros_like(ref)
                _fused.render_fwd_hip(*g, cam, bg, 32, row_range=(r0, r1), out=buf, info=info, rows16=True)
                assert info["flags"] & 2048, (label, world, r)
                assert info["on_grid"] < full["on_grid"], (label, world, r, info["on_grid"], full["on_grid"])
                regime.setdefault(f"{label}/world{world}", []).append(full["on_grid"] - info["on_grid"])
    print("REGIME band pre-cull: candidates removed per band", regime, "edge Gaussians", n_edge)


# ------------------------------------------------------------------ e. intrinsics that change from frame to frame
def test_frames_whose_intrinsics_change_with_the_depth_cut(device):
    """Twelve frames at a still pose that zoom (fx and fy together, then fx alone, then fy alone) and pan the principal
    point, on 32-px bins with the depth cut forced (lazy sorting, speculation): every frame equals the per-stage frame
    bit for bit, and the last one is within check_image_strict of the oracle."""
    _hip_mod.config_depth_cut(2)
    W, H = 480, 272
    cam0 = general_camera(W, H, 420.0, 336.0, 0.33 * W, 0.65 * H, near=0.5, far=30.0)
    sc, _ = general_scene(cam0, n_view=150_000, n_side=40, seed=50, view_scale=(0.02, 0.08))
    sc = {k: v.to(device) for k, v in sc.items()}
    bg = torch.tensor(BG, device=device)
    R, T = cam0.R.to(device), cam0.T.to(device)
    intr = []
    for k in range(12):
        fx, fy, cx, cy = 420.0, 336.0, 0.33 * W, 0.65 * H
        if k < 4:
            fx, fy = fx * (1 + 0.04 * k), fy * (1 + 0.04 * k)
        elif k < 6:
            fx = fx * (1 + 0.05 * (k - 3))
        elif k < 8:
            fy = fy * (1 - 0.05 * (k - 5))
        else:
            cx, cy = cx - 9.0 * (k - 7), cy + 6.0 * (k - 7)
        intr.append((fx, fy, cx, cy))
    _fused._state.clear()
    _fused.FRAME_STATS = st = {}
    try:
        for k, (fx, fy, cx, cy) in enumerate(intr):
            cm = Camera(R=R, T=T, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.5, far=30.0)
            assert_general_camera(cm)
            got = ms.render_gaussians(*_args(sc), cm, background_color=bg, bin_size=32)
            want = _stagewise(sc, cm, bg, 16)
            assert torch.equal(got, want), (k, (fx, fy, cx, cy), dict(st), float((got - want).abs().max()))
    finally:
        _fused.FRAME_STATS = None
        _fused._state.clear()
    print("REGIME intrinsics sequence frame stats", st)
    assert st.get("depth_cut", 0) > 0, st
    _assert_clamped(sc, cam0, oracle_project(oracle, *[sc[k].cpu() for k in NAMES[:4]], cam0)[3], "intrinsics sequence, frame 0")
    ref, aux = _oracle_frame(sc, cm, BG)
    check_image_strict(got, ref, aux["margin"], tag="cameras/intrinsics-sequence", eps=2e-5)


# ------------------------------------------------------------------ f. backward
BWD_CASES = [("lean", 3, {}), ("lean_densify", 3, {"densify": True}), ("stagewise", 3, {"stagewise": True}),
             ("stagewise_densify", 3, {"stagewise": True, "densify": True}), ("c8_non_packed", 8, {})]


@pytest.mark.parametrize("name", ["fx>fy_pp_xy", "fy>fx_pp_xy"])
@pytest.mark.parametrize("case,C,kw", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_backward_at_general_cameras(device, name, case, C, kw):
    """render_gaussians_trainable against float64 autograd of torch_oracle.project + rasterize on the HIP forward's own
    lists, with test_hip_backward_paths.py's branch guard and bars.  lean: k_rasterize_bwd_quads + project_bwd_from_rows;
    lean_densify: the densify STATS finish (ms_render_bwd_finish_densify); stagewise: ms_project_gaussians_bwd;
    c8_non_packed: ms_render_bwd's non-packed branch (ms_project_gaussians_bwd with radii).  Densification statistics
    against densify.update_torch on the float64 dL/dmeans2d (count, max_radii exactly)."""
    # (no Gaussians at the near plane here: at z ~ 0.5 their fp32 gradients keep fewer digits than the bars ask of every
    # element -- on every backward path alike; the planes' culling is tested by the forward tests above)
    sc, _, cam = _scene(name, device, seed=60 + C, channels=C, n_view=500, n_plane=0)
    H, W, ts = cam.H, cam.W, 16
    bg = (torch.rand(C, generator=torch.Generator().manual_seed(7)) * 0.6 + 0.1).to(device)
    leaves = [sc[k].clone().requires_grad_(True) for k in NAMES]
    with torch.no_grad():
        m2h, conh, deph, radh = project_gaussians_autograd(*[l.detach() for l in leaves[:4]], cam)
        ids, ranges = bin_gaussians_to_tiles_hip(m2h, radh, deph, ts, -(-W // ts), -(-H // ts))
    counts = _assert_clamped(sc, cam, radh, f"{name}/{case}")
    ids_c, ranges_c = np_(ids).astype(np.int32), np_(ranges).astype(np.int32)
    up = Upstream(np_(m2h), np_(conh), np_(sc["features"]), np_(sc["opacities"]), bg.cpu(), ranges_c, ids_c, H, W, ts, seed=61)
    print("REGIME", name, case, "guarded pixels", int(up.guard.sum()), "of", up.guard.size)
    st = DensifyStats(sc["means3d"].shape[0], device) if kw.get("densify") else None
    img = render_gaussians_trainable(*leaves, cam, background_color=bg, tile_size=ts, stagewise=kw.get("stagewise", False),
                                     densify=st)
    img.backward(up.v_img.to(device))
    torch.cuda.synchronize()
    rl = [l.detach().cpu().double().requires_grad_(True) for l in leaves]
    rbg = bg.detach().cpu().double()
    rm2, rcon, _ = torch_oracle.project(rl[0], rl[1], rl[2], cam.view_matrix.cpu().double(), cam.fx, cam.fy, cam.cx, cam.cy, W, H)
    rm2.retain_grad()
    rimg, _ = torch_oracle.rasterize(rm2, rcon, rl[4], rl[3], rbg, torch.from_numpy(ranges_c), torch.from_numpy(ids_c), H, W, ts)
    assert np.abs(np_(img) - rimg.detach().numpy())[~up.guard].max() <= 2e-4
    (rimg * up.v_img.double()).sum().backward()
    tag = f"cameras/{name}/{case}/C{C}"
    for n_, a, b in zip(NAMES, leaves, rl):
        assert_grad_close(f"{tag}/{n_}", a.grad, b.grad, rel=5e-3, elem_rel=ELEM_F64)
    if st is not None:
        ref = update_torch(DensifyStats(rm2.shape[0], "cpu"), rm2.grad, radh.cpu(), W, H)
        assert torch.equal(st.count.cpu(), ref.count), f"{tag}: count"
        assert torch.equal(st.max_radii.cpu(), ref.max_radii), f"{tag}: max_radii"
        assert_grad_close(f"{tag}/grad2d", st.grad2d.cpu(), ref.grad2d, **F64_2D)
