"""No cached state outlives an in-place update of its tensors.

The package caches by "same tensor object, same ``_version``" (the band path's ms_scene, a prepared scene's block bounds, a
camera's float32 matrix and centre), and autograd checks its saved tensors the same way.  Its own HIP writers change
tensors through raw pointers, so each of them has to move the version counter itself (``_hip.bump``), and a storage swap
(``t.data = other``) keeps object and version, so the caches look at the data pointer too.

Every frame comparison here is against a COLD frame: the same values as fresh tensor objects and a fresh ``Camera`` built
from a clone of the matrix, through blocking ``render_gaussians(backend="hip")`` -- the path the rest of the suite holds to
the oracle.  Warm and cold run the same kernels on the same bits (tests/test_hip_fused.py establishes band-assembled ==
blocking, bit for bit), so the comparison is ``torch.equal``; and every test asserts that the update mattered (the warm
frame before it differs from the cold frame after it), so a stale cache cannot pass by accident."""
import gc

import numpy as np
import pytest
import torch

import mojosplat_amd as ms
import oracle
from mojosplat_amd import GaussianAdam, _band, scene_order
from mojosplat_amd.autograd import render_gaussians_trainable
from mojosplat_amd.densify import DensifyStats, update_torch
from mojosplat_amd.distributed import _render_band, render_gaussians_sharded
from mojosplat_amd.mcmc import inject_noise, relocate_dead
from mojosplat_amd.scene_order import prepare_scene, prepared_bounds
from mojosplat_amd.scenes import BACKGROUND_V1, randscene_v1
from mojosplat_amd.utils import Camera

pytestmark = pytest.mark.gpu

NAMES = ("means3d", "scales", "quats", "opacities", "features")


# ------------------------------------------------------------------ cold frames, band frames
def _cold_camera(cam):
    vm = cam.view_matrix.detach().clone()
    return Camera(R=vm[:3, :3].contiguous(), T=vm[:3, 3].contiguous(), H=cam.H, W=cam.W, fx=cam.fx, fy=cam.fy, cx=cam.cx,
                  cy=cam.cy, near=cam.near, far=cam.far, view_matrix=vm)


def _cold_frame(g, cam, bg, **kw):
    with torch.no_grad():
        return ms.render_gaussians(*[t.detach().clone() for t in g], _cold_camera(cam), background_color=bg, backend="hip", **kw)


def _band_frame(g, cam, bg, world):
    """The frame assembled from the `world` rehearsed ranks' bands of the sharded entry point (the cached ms_scene path)."""
    th = -(-cam.H // 16)
    rows = -(-th // world)
    frame = None
    for r in range(world):
        band = render_gaussians_sharded(*g, cam, background_color=bg, rehearse=(r, world))
        frame = torch.full_like(band, -1.0) if frame is None else frame
        y0, y1 = min(r * rows * 16, cam.H), min((r + 1) * rows * 16, cam.H)
        frame[y0:y1] = band[y0:y1]
    return frame


def _changed(a, b):
    """Fraction of the pixels in which two frames differ."""
    return float((a != b).any(-1).float().mean())


# ------------------------------------------------------------------ a. every writer moves the version counters
N_ROWS = 257      # one full 256-row block of the kernels plus a ragged row


def _rows_scene(device, seed=3):
    """257 Gaussians in front of randscene_v1's camera, a third of them dead (opacity under MCMC's 0.005), linear opacities."""
    g = torch.Generator().manual_seed(seed)
    sc, cam = randscene_v1(N_ROWS, 64, 48, ell=-2.0, seed=seed, device=device)
    sc["opacities"][(torch.rand(N_ROWS, generator=g) < 0.33).to(device)] = 0.001
    return sc, cam


def _adam_case(device, backend, masked):
    g = torch.Generator().manual_seed(7)
    params = {"a": torch.randn(N_ROWS, 3, generator=g), "b": torch.randn(N_ROWS, 4, generator=g), "frozen": torch.randn(N_ROWS, generator=g)}
    params = {k: v.to(device).requires_grad_() for k, v in params.items()}
    opt = GaussianAdam(params, lr=1e-2, backend=backend)
    grads = {k: torch.randn(v.shape, generator=g).to(device) for k, v in params.items()}
    vis = (torch.arange(N_ROWS) % 3 != 0).to(device) if masked else None
    for k in params:
        params[k].grad = grads[k].clone()
    opt.step(visibility=vis)                      # (the moments exist from here on)
    params["frozen"].grad = None                  # a parameter without a gradient: nobody touches it or its moments
    watch = dict(params)
    for k, p in params.items():
        watch[k + ".exp_avg"], watch[k + ".exp_avg_sq"] = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
    return watch, lambda: opt.step(visibility=vis)


def _relocate_case(device, backend):
    sc, _ = _rows_scene(device)
    params = {k: v.requires_grad_() for k, v in sc.items()}
    opt = GaussianAdam(params, lr=1e-3, backend=backend)
    g = torch.Generator().manual_seed(11)
    for p in params.values():
        p.grad = torch.randn(p.shape, generator=g).to(device)
    opt.step()
    watch = dict(params)
    for k, p in params.items():
        watch[k + ".exp_avg"], watch[k + ".exp_avg_sq"] = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
    draws = torch.rand(N_ROWS, generator=g, dtype=torch.float64).to(device)
    watch["draws"] = draws                        # (an input: read, never written)

    def run():
        res = relocate_dead(params, opt, opacity_space="linear", draws=draws, backend=backend)
        assert 0 < int(res.n) < N_ROWS, "the case has dead rows and live ones"
    return watch, run


def _noise_case(device, backend):
    sc, _ = _rows_scene(device)
    noise = torch.randn(N_ROWS, 3, generator=torch.Generator().manual_seed(5)).to(device)
    return dict(sc), lambda: inject_noise(sc, 1e-3, opacity_space="linear", noise=noise, backend=backend)


def _densify_case(device, backend, stagewise):
    """backend="hip": the training backward with densify=stats (the fused frame's finish kernel, or the per-stage
    path's ms_densify_stats_update); backend="torch": densify.update_torch, the definition, on arrays of its own (random
    v_means2d and radii of the same shapes, seed 9: some rows alive, some not -- moved / not moved does not depend on the
    values, and update_torch's index assignments move the counters even where no row is alive)."""
    sc, cam = _rows_scene(device)
    stats = DensifyStats(N_ROWS, device)
    watch = dict(grad2d=stats.grad2d, count=stats.count, max_radii=stats.max_radii, **sc)
    if backend == "torch":
        g = torch.Generator().manual_seed(9)
        v_means2d = torch.randn(N_ROWS, 2, generator=g)
        radii = torch.randint(0, 5, (N_ROWS, 2), generator=g, dtype=torch.int32)
        return watch, lambda: update_torch(stats, v_means2d, radii, cam.W, cam.H)
    leaves = [sc[k].requires_grad_() for k in NAMES]

    def run():
        img = render_gaussians_trainable(*leaves, cam, background_color=torch.tensor(BACKGROUND_V1, device=device),
                                            stagewise=stagewise, densify=stats)
        img.square().mean().backward()
        assert float(stats.count.sum()) > 0, "the view saw Gaussians: the kernel wrote the statistics"
    return watch, run


WRITERS = {
    "adam_dense": lambda dev, be: _adam_case(dev, be, False),
    "adam_masked": lambda dev, be: _adam_case(dev, be, True),
    "relocate_dead": _relocate_case,
    "inject_noise": _noise_case,
    "backward_densify_fused": lambda dev, be: _densify_case(dev, be, False),
    "backward_densify_stagewise": lambda dev, be: _densify_case(dev, be, True),
}


@pytest.mark.parametrize("writer", list(WRITERS))
def test_every_in_place_hip_writer_moves_the_version_counters(device, writer):
    """For every tensor a backend="hip" call may write in place: its ``_version`` moves exactly where the same call with
    backend="torch" (the definition) on CPU tensors moves it, and stays where the definition leaves it -- a parameter whose
    ``grad`` is None and its moments, the scales / quats / opacities under ``inject_noise``, the Gaussians under a backward
    that accumulates densification statistics.  Moved / not moved is compared, not the counts."""
    moved = {}
    for backend, dev in (("torch", torch.device("cpu")), ("hip", device)):
        watch, run = WRITERS[writer](dev, backend)
        before = {k: t._version for k, t in watch.items()}
        run()
        moved[backend] = {k: watch[k]._version > before[k] for k in watch}
    assert moved["hip"].keys() == moved["torch"].keys()
    assert any(moved["torch"].values()) and not all(moved["torch"].values()), "the case has tensors of both kinds"
    wrong = {k: (moved["hip"][k], moved["torch"][k]) for k in moved["torch"] if moved["hip"][k] != moved["torch"][k]}
    assert not wrong, f"{writer}: (hip moved, torch moved) differ for {wrong}"


# ------------------------------------------------------------------ b. autograd's saved-tensor check
@pytest.mark.parametrize("backend", ["torch", "hip"])
def test_backward_through_a_graph_from_before_the_step_raises(device, backend):
    """A graph that saved ``p`` before the optimiser step must not be differentiated after it: autograd notices through the
    version counter (``backend="torch"``, the control, moves it with ``copy_``).  A HIP step that left the counter alone
    would hand back the gradient of the wrong point without a word."""
    p = torch.randn(64, 3, generator=torch.Generator().manual_seed(1)).to(device).requires_grad_()
    y = (p * p).sum()
    y.backward(retain_graph=True)
    before = p.detach().clone()
    GaussianAdam({"p": p}, lr=1e-2, backend=backend).step()
    assert not torch.equal(p.detach(), before), "the step moved p"
    with pytest.raises(RuntimeError, match="inplace"):
        y.backward()


# ------------------------------------------------------------------ c. a prepared scene trained with HIP Adam
@pytest.mark.parametrize("N", [4096, 40_960])
def test_prepared_scene_trained_with_hip_adam_drops_its_bounds(device, N):
    """A PREPARED scene (Morton order, the bounds of every block of 256) is rendered through the band path until its ms_scene
    and the one-entry fast path are warm, then trained for three iterations -- differentiable frame, photometric loss,
    backward, ``GaussianAdam(backend="hip").step()``, the second one masked by the view's radii.  After every step the
    bounds are gone (``prepared_bounds`` is None: the means have left their boxes) and the band-assembled frame equals the
    cold frame of the same values bit for bit.

    N = 4096 (16 blocks, 13 tile rows) is the cached-struct case.  N = 40 960 is past the library's threshold for the band
    pre-cull (32 768 Gaussians, a band under 60 % of the rows): there a rank that kept the stale bounds skips blocks by
    boxes their Gaussians have left and pre-culls by their old means.

    The means' learning rate comes from the scene: Adam's first step moves every coordinate that has a gradient by ``lr``,
    and ``lr`` = the median over the blocks of a box's longest side takes such a Gaussian out of its block's box along
    every axis.  Asserted from the cold reference alone: at least a quarter of the Gaussians lie outside their block's
    old box after the first step, the frame after it is not all background and differs from the frame before it in at
    least 1 % of the pixels."""
    W, H, world = 320, 200, 4
    sc, cam = randscene_v1(N, W, H, ell=-2.5 if N == 4096 else -3.2, seed=17, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    ps = prepare_scene(*[sc[k] for k in NAMES])
    g = ps.arrays
    assert ps.block_bounds.shape == (N // 256, 8) and -(-H // 16) == 13
    for t in g:
        t.requires_grad_()
    assert prepared_bounds(g[0], g[1]) is not None, "requires_grad_ keeps object, version and storage: still prepared"
    old_bounds = ps.block_bounds.clone()
    lr = float((old_bounds[:, 4:7] - old_bounds[:, 0:3]).max(1).values.median())
    blk = torch.arange(N, device=device) // 256

    warm = _band_frame(g, cam, bg, world)
    assert torch.equal(_band_frame(g, cam, bg, world), warm)               # (the second pass: the fast path)
    assert _band.scene_struct(*g).block_bounds == ps.block_bounds.data_ptr(), "the warm ms_scene carries the bounds"
    cold0 = _cold_frame(g, cam, bg)
    assert torch.equal(warm, cold0)

    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(23)).to(device)
    opt = GaussianAdam(dict(zip(NAMES, g)), lr={"means3d": lr, "scales": 5e-3, "quats": 1e-3, "opacities": 1e-2, "features": 2.5e-3},
                       backend="hip")
    prev_cold = cold0
    for it in range(3):
        img = render_gaussians_trainable(*g, cam, background_color=bg)
        ms.photometric_loss(img, target).backward()
        vis = None
        if it == 1:
            with torch.no_grad():
                radii = ms.project_gaussians(*g[:4], cam, backend="hip")[3]
            vis = (radii > 0).all(-1)
            assert 0 < int(vis.sum()) < N, "the mask hides some Gaussians and shows others"
        opt.step(visibility=vis)
        opt.zero_grad()
        assert prepared_bounds(g[0], g[1]) is None, f"step {it}: the means moved under the bounds"
        cold = _cold_frame(g, cam, bg)
        if it == 0:
            m = g[0].detach()
            outside = float(((m < old_bounds[blk, 0:3]) | (m > old_bounds[blk, 4:7])).any(1).float().mean())
            moved_px, lit = _changed(cold, cold0), float((cold != bg).any(-1).float().mean())
            assert outside >= 0.25 and moved_px >= 0.01 and lit > 0.0, \
                f"lr {lr:.4f}: outside their old box {outside:.3f}, pixels changed {moved_px:.3f}, not background {lit:.3f}"
        assert _changed(warm if it == 0 else prev_cold, cold) > 0.0, f"step {it} changed the frame"
        got = _band_frame(g, cam, bg, world)
        assert torch.equal(got, cold), f"step {it}: {_changed(got, cold):.4f} of the band-assembled pixels differ from the cold frame"
        assert _band.scene_struct(*g).block_bounds is None
        prev_cold = cold


# ------------------------------------------------------------------ d. a pose trained with HIP Adam
def test_pose_trained_with_hip_adam_keeps_one_camera_per_frame(device):
    """``view_matrix`` is a float32 leaf on the device, the ``Camera`` object is kept across steps and
    ``GaussianAdam({"pose": vm}, backend="hip")`` updates it through its raw pointer.  ``Camera._viewmat_f32`` aliases the
    matrix (the projection reads the new pose at once) while ``Camera._campos`` caches host floats: after each of three
    steps the SH colours through the kept camera equal a cold camera's bit for bit and lie within tests/test_sh.py's 5e-6 of
    the float64 oracle at the cold camera's centre, the no-grad frame through the kept camera equals the cold frame, and
    the matrix's bottom row is still [0, 0, 0, 1] (its gradient is zero, and Adam leaves a zero-gradient entry alone).
    lr = 0.02 per step and entry: the centre -R^T T moves by at least 0.05 scene units over the three steps (asserted from
    the float64 centre) -- colours then change by far more than the bar."""
    N, lr = 2000, 0.02
    sc, cam0 = randscene_v1(N, 128, 128, ell=-3.0, seed=29, device=device)
    coeffs = (torch.randn(N, 9, 3, generator=torch.Generator().manual_seed(31)) * 0.5).to(device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = [sc[k] for k in NAMES[:4]]
    vm = cam0.view_matrix.detach().clone().requires_grad_()
    assert vm.dtype == torch.float32 and vm.is_contiguous() and vm.is_leaf
    cam = Camera(R=cam0.R, T=cam0.T, H=cam0.H, W=cam0.W, fx=cam0.fx, fy=cam0.fy, cx=cam0.cx, cy=cam0.cy, near=cam0.near,
                 far=cam0.far, view_matrix=vm)
    far_cam = Camera(R=cam0.R, T=cam0.T + torch.tensor([0.3, -0.2, 0.4], device=device), H=cam0.H, W=cam0.W, fx=cam0.fx,
                     fy=cam0.fy, cx=cam0.cx, cy=cam0.cy, near=cam0.near, far=cam0.far)
    with torch.no_grad():
        target = ms.render_gaussians(*g, coeffs, far_cam, sh_degree=2, background_color=bg, backend="hip")

    def centre64():
        m = vm.detach().double().cpu().numpy()
        return -(m[:3, :3].T @ m[:3, 3])

    def frame_and_colours(camera):
        with torch.no_grad():
            return (ms.render_gaussians(*g, coeffs, camera, sh_degree=2, background_color=bg, backend="hip"),
                    ms.evaluate_sh(g[0], coeffs, camera, 2))

    warm_frame, warm_col = frame_and_colours(cam)       # (both caches of the kept camera are warm)
    c_start = centre64()
    opt = GaussianAdam({"pose": vm}, lr=lr, backend="hip")
    means_np, coeffs_np = g[0].cpu().numpy(), coeffs.cpu().numpy()
    for it in range(3):
        img = render_gaussians_trainable(*g, coeffs, cam, background_color=bg, sh_degree=2)
        (img - target).abs().mean().backward()
        assert vm.grad is not None and bool((vm.grad[3] == 0).all()) and float(vm.grad[:3].abs().max()) > 0
        opt.step()
        opt.zero_grad()
        cold_cam = _cold_camera(cam)
        cold_frame, cold_col = frame_and_colours(cold_cam)
        got_frame, got_col = frame_and_colours(cam)
        assert torch.equal(got_col, cold_col), f"step {it}: colours from a stale camera centre, max {float((got_col - cold_col).abs().max()):.3g}"
        want = oracle.sh_fwd(means_np, centre64(), coeffs_np, 2)
        err = float(np.abs(got_col.cpu().numpy() - want).max())
        assert err < 5e-6, (it, err)
        assert torch.equal(got_frame, cold_frame), f"step {it}: {_changed(got_frame, cold_frame):.4f} of the pixels differ from the cold frame"
        assert torch.equal(vm.detach()[3], torch.tensor([0.0, 0.0, 0.0, 1.0], device=device))
        assert _changed(warm_frame, cold_frame) > 0.0 and float((cold_col - warm_col).abs().max()) > 100 * 5e-6
    moved = float(np.linalg.norm(centre64() - c_start))
    assert moved >= 0.05, f"the centre moved by {moved:.4f}"


# ------------------------------------------------------------------ e. storage swaps
def test_storage_swaps_reach_the_band_path_and_the_camera(device):
    """``t.data = other`` keeps the tensor object AND its version counter (``t.set_(other)`` the object): the band path's
    cached ms_scene and the camera's cached matrix must follow the data pointer.  The old storage stays referenced, so a
    stale read lands in live memory that holds the old values -- never in freed memory."""
    N, W, H, world = 1000, 128, 96, 2
    sc, cam0 = randscene_v1(N, W, H, ell=-2.5, seed=37, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = [sc[k] for k in NAMES]
    cam = _cold_camera(cam0)
    kept_alive = []

    def swap(t, new, how):
        kept_alive.append(t.detach()[:])                 # (a view of the OLD storage)
        version = t._version
        if how == "data":
            t.data = new
            assert t._version == version
        else:
            t.set_(new)
        assert t.data_ptr() == new.data_ptr() != kept_alive[-1].data_ptr()

    swaps = [
        ("means3d.data", lambda: swap(g[0], g[0].detach() + torch.tensor([0.4, -0.3, 0.2], device=device), "data")),
        ("scales.set_", lambda: swap(g[1], g[1].detach() + 0.5, "set_")),
        ("view_matrix.data", lambda: swap(cam.view_matrix, _moved_pose(cam.view_matrix), "data")),
    ]
    for name, do in swaps:
        warm = _band_frame(g, cam, bg, world)
        assert torch.equal(_band_frame(g, cam, bg, world), warm)           # (twice: warm)
        do()
        cold = _cold_frame(g, cam, bg)
        assert _changed(warm, cold) >= 0.01, f"{name}: the swap changed the frame"
        got = _band_frame(g, cam, bg, world)
        assert torch.equal(got, cold), f"{name}: {_changed(got, cold):.4f} of the band-assembled pixels differ from the cold frame"
        with torch.no_grad():
            assert torch.equal(ms.render_gaussians(*g, cam, background_color=bg, backend="hip"), cold), name


def _moved_pose(vm):
    out = vm.detach().clone()
    out[:3, 3] += torch.tensor([0.3, 0.2, -0.5], device=vm.device)
    return out


# ------------------------------------------------------------------ f. release_scratch
def test_release_scratch_leaves_a_prepared_scene_prepared(device):
    """``release_scratch()`` hands the render scratch and the cached ms_scenes back; a live ``PreparedScene`` keeps its bounds
    (the registry holds weak references only: nothing is gained by clearing it, and nothing registers a scene again).  The
    band's candidate count after the pre-cull -- the first number of the band's size record -- is the same before and after,
    the ms_scene built after the call carries the bounds again, the frame equals the blocking frame; and the registry's
    entry goes with the scene.  N = 40 960: the library pre-culls bands from 32 768 Gaussians on."""
    N, W, H, world = 40_960, 320, 200, 4
    sc, cam = randscene_v1(N, W, H, ell=-3.2, seed=41, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    ps = prepare_scene(*[sc[k] for k in NAMES])
    g = ps.arrays
    key = id(g[0])
    ref = ms.render_gaussians(*g, cam, background_color=bg, backend="hip")
    assert float((ref != bg).any(-1).float().mean()) > 0.01

    def candidates(band):
        out = torch.zeros_like(ref)
        on_grid, pairs, culled = _render_band(None, *g, cam, bg, 16, band, out)
        assert culled, "the library pre-culled the band"
        return on_grid, pairs

    band = (4, 8)
    before = candidates(band)
    assert 0 < before[0] < N
    assert _band.scene_struct(*g).block_bounds == ps.block_bounds.data_ptr()
    ms.release_scratch()
    assert not _band._scenes
    pb = prepared_bounds(g[0], g[1])
    assert pb is not None and pb[0] is ps.block_bounds and pb[1] == ps.block_size
    assert candidates(band) == before
    assert _band.scene_struct(*g).block_bounds == ps.block_bounds.data_ptr(), "the rebuilt ms_scene has the bounds"
    assert torch.equal(_band_frame(g, cam, bg, world), ref)
    # a dropped scene takes its entry along (the lanes' cached frame structs and ms_scenes held the arrays until here)
    assert key in scene_order._registry
    ms.release_scratch()
    del ps, g, pb, candidates
    gc.collect()
    assert key not in scene_order._registry
