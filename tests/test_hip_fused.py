"""GPU: the one-call forward path (ms_render_fwd, what render_gaussians(backend='hip') runs)
is bit-identical to the three per-stage calls, across buffer growth, empty scenes, fp16
colours and tile sizes."""
import math
import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import _fused
from mojosplat_amd import _hip as _hip_mod
from mojosplat_amd.scenes import BACKGROUND_V1, randscene_v1

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_depth_cut_after_each_test():
    """Tests switch the library's depth-cut mode in-process (ms_config_depth_cut: the environment is read once); every
    test leaves the default behind."""
    yield
    _hip_mod.config_depth_cut(1, 6_000_000)


def stagewise(sc, cam, bg, tile_size=16):
    m2, con, dep, rad = ms.project_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], cam,
                                             backend="hip")
    ids, ranges = ms.bin_gaussians_to_tiles(m2, rad, dep, cam.H, cam.W, tile_size, backend="hip")
    if ids.numel() == 0:
        return torch.zeros(cam.H, cam.W, sc["features"].shape[1], device=m2.device)
    return ms.rasterize_gaussians(m2, con, sc["features"], sc["opacities"], bg, ranges, ids, cam,
                                  tile_size=tile_size, backend="hip")


@pytest.mark.parametrize("N,W,H,ell,ts", [(3000, 320, 200, -2.5, 16), (50_000, 640, 360, -3.5, 16),
                                          (2000, 128, 96, -2.0, 8), (2000, 160, 96, -2.0, 32)])
def test_fused_equals_stagewise(device, N, W, H, ell, ts):
    _fused._state.clear()  # start from no scratch: exercises workspace + intersection-buffer growth
    sc, cam = randscene_v1(N, W, H, ell=ell, seed=N, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    a = ms.render_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"], cam,
                            background_color=bg, tile_size=ts, backend="hip")
    b = stagewise(sc, cam, bg, ts)
    assert torch.equal(a, b)
    # second frame reuses the cached scratch; a larger scene then forces a regrow
    a2 = ms.render_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"], cam,
                             background_color=bg, tile_size=ts, backend="hip")
    assert torch.equal(a, a2)
    sc2, cam2 = randscene_v1(4 * N, W, H, ell=ell + 0.5, seed=N + 1, device=device)
    a3 = ms.render_gaussians(sc2["means3d"], sc2["scales"], sc2["quats"], sc2["opacities"], sc2["features"], cam2,
                             background_color=bg, tile_size=ts, backend="hip")
    assert torch.equal(a3, stagewise(sc2, cam2, bg, ts))


def test_fused_empty_scene_is_zeros_and_fp16_colours(device):
    sc, cam = randscene_v1(1000, 160, 96, ell=-2.5, seed=3, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    away = sc["means3d"] + torch.tensor([0.0, 0.0, -800.0], device=device)
    img = ms.render_gaussians(away, sc["scales"], sc["quats"], sc["opacities"], sc["features"], cam,
                              background_color=bg, backend="hip")
    assert img.shape == (96, 160, 3) and (img == 0).all()
    sc16 = dict(sc, features=sc["features"].half())
    a = ms.render_gaussians(sc16["means3d"], sc16["scales"], sc16["quats"], sc16["opacities"], sc16["features"],
                            cam, background_color=bg, backend="hip")
    assert a.dtype == torch.float32
    # render_gaussians casts the background to the colour dtype, like the reference (render.py:52-55)
    assert torch.equal(a, stagewise(sc16, cam, bg.half()))


def test_band_calls_assemble_the_full_frame(device):
    """The multi-GPU decomposition on one GPU: ms_render_fwd per tile-row band into one shared
    framebuffer == the whole-image call, and the world=1 sharded entry point == render_gaussians."""
    from mojosplat_amd.distributed import band_plan, render_gaussians_sharded
    sc, cam = randscene_v1(30_000, 640, 360, ell=-3.0, seed=9, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    ref = ms.render_gaussians(*g, cam, background_color=bg, backend="hip")
    th = -(-cam.H // 16)
    for world in (2, 3, 8):
        rows, bands = band_plan(th, world)
        frame = torch.full((max(world * rows * 16, cam.H), cam.W, 3), -1.0, device=device)
        total = 0
        for band in bands:
            if band[1] > band[0]:
                _, m = _fused.render_fwd_hip(*g, cam, bg, 16, row_range=band, out=frame)
                total += m
        assert torch.equal(frame[:cam.H], ref)
        assert (frame[cam.H:] == -1.0).all()      # padding rows are never written
    assert torch.equal(render_gaussians_sharded(*g, cam, background_color=bg), ref)
    assert torch.equal(render_gaussians_sharded(*g, cam, background_color=bg, async_op=True).wait(), ref)


def test_sharded_path_tells_a_prefix_view_from_its_scene(device):
    """Round-6 advisor finding: `means3d[:k]` shares its base's data pointer and version counter, so the cached ms_scene of
    the full scene must not be handed to a render of the prefix (or the reverse): every call through the sharded path equals
    the single-GPU frame of exactly the arrays it was given."""
    from mojosplat_amd.distributed import band_plan, render_gaussians_sharded
    sc, cam = randscene_v1(20_000, 480, 272, ell=-3.0, seed=3, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    for k in (20_000, 5_000, 20_000, 64, 5_000):
        gk = tuple(t[:k] for t in g)
        ref = ms.render_gaussians(*gk, cam, background_color=bg, backend="hip")
        assert torch.equal(render_gaussians_sharded(*gk, cam, background_color=bg), ref), k
        assert torch.equal(render_gaussians_sharded(*gk, cam, background_color=bg, async_op=True).wait(), ref), k
        rows, bands = band_plan(-(-cam.H // 16), 2)
        for r, (r0, r1) in enumerate(bands):
            y0, y1 = min(r0 * 16, cam.H), min(r1 * 16, cam.H)
            band = render_gaussians_sharded(*gk, cam, background_color=bg, rehearse=(r, 2))
            assert torch.equal(band[y0:y1], ref[y0:y1]), (k, r)
    # an in-place update that does not bump the version counter is the caller's to announce (release_scratch); one that does
    # is noticed
    g[0].add_(0.25)
    ref = ms.render_gaussians(*g, cam, background_color=bg, backend="hip")
    assert torch.equal(render_gaussians_sharded(*g, cam, background_color=bg), ref)
    # a PendingFrame dropped unwaited gives its lane back and the next frames are unharmed
    for _ in range(3):
        render_gaussians_sharded(*g, cam, background_color=bg, async_op=True)
    assert torch.equal(render_gaussians_sharded(*g, cam, background_color=bg, async_op=True).wait(), ref)


def test_sharded_bands_with_an_explicit_tile_size_and_on_sparse_scenes(device):
    """(1) render_gaussians_sharded(tile_size=32 / 64): band plan, slab and the band handed to the library are in
    rows of THAT tile size (the 16-px-row mode belongs to rule-chosen bins under 16-px tiles only) -- every rehearsed
    rank's slab equals the single-GPU frame's rows.  (2) A rehearsed rank whose band no Gaussian reaches returns
    its band as background, not the frame-level zeros image (the pre-culled on-grid count cannot decide that rule)."""
    from mojosplat_amd.distributed import band_plan, render_gaussians_sharded
    sc, cam = randscene_v1(30_000, 640, 360, ell=-3.0, seed=9, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    ref = ms.render_gaussians(*g, cam, background_color=bg, backend="hip")
    for ts in (32, 64):
        th = -(-cam.H // ts)
        for world in (2, 3):
            rows, bands = band_plan(th, world)
            for r, (r0, r1) in enumerate(bands):
                y0, y1 = min(r0 * ts, cam.H), min(r1 * ts, cam.H)
                a = render_gaussians_sharded(*g, cam, background_color=bg, tile_size=ts, rehearse=(r, world))
                b = render_gaussians_sharded(*g, cam, background_color=bg, tile_size=ts, async_op=True,
                                             rehearse=(r, world)).wait()
                assert torch.equal(a[y0:y1], ref[y0:y1]) and torch.equal(b[y0:y1], ref[y0:y1]), (ts, world, r)
    # a scene that only reaches the top of the image: the lower bands hold nothing
    m2, _, _, rad = ms.project_gaussians(*g[:4], cam, backend="hip")
    top = (rad[:, 1] > 0) & (m2[:, 1] + rad[:, 1].float() < 150.0)      # footprints that end above row 150
    assert 1000 < int(top.sum()) < 30_000
    g2 = tuple(t[top].contiguous() for t in g)
    ref2 = ms.render_gaussians(*g2, cam, background_color=bg, backend="hip")
    assert (ref2[-32:] == bg).all() and not (ref2 == bg).all()
    world = 4
    rows, bands = band_plan(-(-cam.H // 16), world)
    out = torch.zeros_like(ref2)
    for r, (r0, r1) in enumerate(bands):
        img = render_gaussians_sharded(*g2, cam, background_color=bg, rehearse=(r, world))
        y0, y1 = min(r0 * 16, cam.H), min(r1 * 16, cam.H)
        out[y0:y1] = img[y0:y1]
    assert torch.equal(out, ref2)


def test_lean_frames_on_wide_grids_and_small_tiles(device):
    """The records a lean frame's count kernel leaves for its scatter kernel: 12 bytes on plain bins of grids up to 255
    tiles a side, 16 + 8 bytes beyond that (here: 8-px tiles across a 2 100-px-wide strip, 263 tiles a row) and on
    split frames; boxes of 33-64 tiles keep every tile under the 12-byte form (large footprints on 8-px tiles).  Every
    form, sync-free and exact, equals the per-stage path bit for bit."""
    bg = torch.tensor(BACKGROUND_V1, device=device)
    for (n, W, H, ell, ts) in ((40_000, 2100, 96, -3.2, 8), (20_000, 640, 360, -2.2, 8), (20_000, 640, 360, -2.2, 32),
                               (30_000, 4128, 64, -3.0, 16)):
        sc, cam = randscene_v1(n, W, H, ell=ell, seed=21, device=device)
        g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
        ref = stagewise(sc, cam, bg, ts)
        for k in range(3):     # exact path (no buffer yet), then two sync-free frames
            img = ms.render_gaussians(*g, cam, background_color=bg, backend="hip", tile_size=ts)
            assert torch.equal(img, ref), (n, W, H, ell, ts, k)


def test_host_threads_render_concurrently_on_their_own_scratch(device):
    """Lane 0 is per host thread: four threads render four different scenes (different sizes and image shapes, so that
    shared scratch would be torn apart) frame after frame at the same time; every frame of every thread equals that
    scene's per-stage frame bit for bit, and each thread ends up with scratch of its own."""
    import threading
    bg = torch.tensor(BACKGROUND_V1, device=device)
    jobs = []
    for k, (n, W, H, ell) in enumerate(((30_000, 640, 360, -3.0), (8_000, 320, 200, -2.5), (60_000, 800, 448, -3.5),
                                          (2_000, 256, 256, -2.0))):
        sc, cam = randscene_v1(n, W, H, ell=ell, seed=30 + k, device=device)
        jobs.append((sc, cam, stagewise(sc, cam, bg, 16)))
    torch.cuda.synchronize()
    errors, scratch = [], []
    # (every thread keeps its scratch until all have reported theirs: a thread that has exited returns its blocks to the
    # allocator, which may hand the same address to a later one -- the comparison below would then see a "shared" pointer)
    alive = threading.Barrier(len(jobs), timeout=120)

    def work(sc, cam, ref):
        try:
            g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
            for i in range(25):
                img = ms.render_gaussians(*g, cam, background_color=bg, backend="hip")
                if not torch.equal(img, ref):
                    errors.append(f"frame {i} of a {g[0].shape[0]}-Gaussian scene differs")
                    return
            scratch.append(_fused._dev_state(g[0].device, 0)["ws"].data_ptr())
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
        finally:
            try:
                alive.wait()
            except threading.BrokenBarrierError:
                pass

    threads = [threading.Thread(target=work, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    assert len(set(scratch)) == len(jobs), "threads shared a workspace"


def test_split_frames_on_bands_that_cut_through_bin_rows(device):
    """Bands of >= 16 tile rows are split frames (32-px bins cut into block lists) even when they start
    or end in the middle of a bin row: the bins of that row are binned whole, only the band's blocks are
    rasterised (and cleaned up).  Thin bands run on 16-px bins.  Together: the whole-image frame."""
    sc, cam = randscene_v1(80_000, 640, 720, ell=-2.7, seed=12, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    ref = stagewise(sc, cam, bg, 16)
    th = -(-cam.H // 16)
    assert th == 45
    for bands in ([(0, 17), (17, 34), (34, 45)], [(0, 21), (21, 45)], [(0, 16), (16, 33), (33, 45)]):
        frame = torch.full((cam.H, cam.W, 3), -1.0, device=device)
        for _ in range(2):   # exact path, then sync-free
            for band in bands:
                _fused.render_fwd_hip(*g, cam, bg, 16, row_range=band, out=frame)
            assert torch.equal(frame, ref), bands
    # the same through the pipelined multi-GPU entry point (each rank's band on a lane stream, two frames
    # in flight), rehearsed rank by rank on this one GPU
    from mojosplat_amd.distributed import band_plan, render_gaussians_sharded
    for world in (2, 3):
        rows, bands = band_plan(th, world)
        for r, (r0, r1) in enumerate(bands):
            a = render_gaussians_sharded(*g, cam, background_color=bg, async_op=True, rehearse=(r, world))
            b = render_gaussians_sharded(*g, cam, background_color=bg, async_op=True, rehearse=(r, world))
            y0, y1 = r0 * 16, min(r1 * 16, cam.H)
            assert torch.equal(a.wait()[y0:y1], ref[y0:y1]) and torch.equal(b.wait()[y0:y1], ref[y0:y1]), (world, r)


def test_band_call_reports_frame_level_on_grid_count(device):
    """isect_info[6]: Gaussians touching the FULL tile grid, the same from every band (also an empty
    one) -- what lets each rank apply the zeros-image rule without a collective."""
    from mojosplat_amd.distributed import _on_grid_count, render_gaussians_sharded
    sc, cam = randscene_v1(20_000, 640, 360, ell=-3.0, seed=2, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    m2, _, _, rad = ms.project_gaussians(*g[:4], cam, backend="hip")
    th, tw = -(-cam.H // 16), -(-cam.W // 16)
    want = _on_grid_count(m2, rad, 16, tw, th)
    assert 0 < want < 20_000
    frame = torch.empty((cam.H, cam.W, 3), device=device)
    for band in ((0, th), (0, 3), (th - 1, th), (5, 5)):
        info = {}
        _fused.render_fwd_hip(*g, cam, bg, 16, row_range=band, out=frame, info=info)
        assert info["on_grid"] == want, band
    # everything behind the camera: zeros, not background, from the sharded entry point too
    far = (sc["means3d"] + torch.tensor([0.0, 0.0, 500.0], device=device),) + g[1:]
    info = {}
    _fused.render_fwd_hip(*far, cam, bg, 16, row_range=(0, 3), out=frame, info=info)
    assert info["on_grid"] == 0
    assert (render_gaussians_sharded(*far, cam, background_color=bg) == 0).all()


def test_multi_view_batch_equals_single_views(device):
    """C cameras in one call (two views in flight on two streams) == C calls."""
    from mojosplat_amd.utils import Camera, look_at
    sc, cam0 = randscene_v1(20_000, 480, 270, ell=-3.0, seed=4, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    cams = []
    for k in range(5):
        vm = look_at(torch.tensor([1.5 * k - 3.0, 1.5, 5.0]), torch.zeros(3), torch.tensor([0.0, 1.0, 0.0])).to(device)
        cams.append(Camera(R=vm[:3, :3].contiguous(), T=vm[:3, 3].contiguous(), H=cam0.H, W=cam0.W, fx=cam0.fx,
                           fy=cam0.fy, cx=cam0.cx, cy=cam0.cy))
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    batch = ms.render_gaussians_batch(*g, cams, background_color=bg)
    assert batch.shape == (5, cam0.H, cam0.W, 3)
    for k, c in enumerate(cams):
        assert torch.equal(batch[k], ms.render_gaussians(*g, c, background_color=bg, backend="hip"))
    assert not torch.equal(batch[0], batch[4])
    # ... and every view against the ORACLE's frame for that camera (the camera dimension the
    # reference's kernels carry, kernels/projection.mojo:32-37), under the suite's strict bar
    import oracle
    from helpers import check_image_strict, np_
    cpu = {k: np_(v) for k, v in sc.items()}
    for k, c in enumerate(cams):
        ref, aux = oracle.render_fwd(cpu["means3d"], cpu["scales"], cpu["quats"], cpu["opacities"], cpu["features"],
                                     np_(c.view_matrix), c.fx, c.fy, c.cx, c.cy, c.W, c.H,
                                     background=np_(bg), margin=True)
        check_image_strict(batch[k], ref, aux["margin"], tag=f"multi-view batch, view {k}", eps=2e-5)


@pytest.fixture
def default_grid_only():
    """render_gaussians without its binning-granularity rule: every frame on the default grid."""
    import os
    from mojosplat_amd import render as R
    old = os.environ.get("MOJOSPLAT_BIN_PX")
    os.environ["MOJOSPLAT_BIN_PX"] = "16"
    R._bin_mode.clear(); R._bin_left.clear()
    yield
    if old is None:
        os.environ.pop("MOJOSPLAT_BIN_PX", None)
    else:
        os.environ["MOJOSPLAT_BIN_PX"] = old
    R._bin_mode.clear(); R._bin_left.clear()


def _stack_scene(n, z_lo, z_hi, opacity, device, seed=0):
    """n big faint Gaussians piled up in front of the camera: every tile of a 64x64 image holds
    thousands of entries and none of them comes close to saturating a pixel."""
    g = torch.Generator().manual_seed(seed)
    means = torch.stack([torch.rand(n, generator=g) * 0.6 - 0.3, torch.rand(n, generator=g) * 0.6 - 0.3,
                         z_lo + (z_hi - z_lo) * torch.rand(n, generator=g)], 1)
    scales = torch.full((n, 3), -0.7) + 0.1 * torch.randn(n, 3, generator=g)
    quats = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=1)
    opac = opacity * (0.8 + 0.4 * torch.rand(n, generator=g))
    cols = torch.rand(n, 3, generator=g)
    from mojosplat_amd.utils import Camera
    cam = Camera(R=torch.eye(3, device=device), T=torch.zeros(3, device=device), H=64, W=64, fx=60.0, fy=60.0,
                 cx=32.0, cy=32.0)
    sc = dict(means3d=means, scales=scales, quats=quats, opacities=opac, features=cols)
    return {k: v.to(device) for k, v in sc.items()}, cam


@pytest.mark.parametrize("n,z_lo,z_hi,opacity,falls_back", [
    (4000, 4.0, 6.0, 0.005, True),       # fronts of 1024 leave T ~ 0.006: every heavy tile is redone
    (6000, 5.0, 5.0, 0.004, False),      # ONE depth, ~2000 per tile: one crowded bucket = the whole list = the front
    (16000, 5.0, 5.0, 0.0055, True),     # ONE depth, > 4096 per tile: no front fits; the clean-up narrows by index
    (3000, 4.0, 4.0001, 0.02, False)])   # a handful of depth values, saturating late
def test_lazy_sorting_clean_up_pass(device, default_grid_only, n, z_lo, z_hi, opacity, falls_back):
    """ms_render_fwd sorts only the front (~1024 nearest entries) of a heavy tile; here that front
    cannot saturate the pixels, so every tile goes through the clean-up kernel (chunked selection,
    including the narrowing into crowded buckets when thousands of entries share one depth).  The
    frame must equal the fully sorted per-stage path bit for bit."""
    from mojosplat_amd.rasterization import rasterize_gaussians_hip
    sc, cam = _stack_scene(n, z_lo, z_hi, opacity, device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    m2, con, dep, rad = ms.project_gaussians(*g[:4], cam, backend="hip")
    ids, ranges = ms.bin_gaussians_to_tiles(m2, rad, dep, cam.H, cam.W, 16, backend="hip")
    ref, alphas, last = rasterize_gaussians_hip(m2, con, g[4], g[3], bg, ranges, ids, cam, 16, return_aux=True)
    counts = (ranges[..., 1] - ranges[..., 0])
    assert counts.max() > 1024
    # some pixel really blended an entry beyond the 1024-entry front of its (heavy) tile
    deepest = (last.view(4, 16, 4, 16).permute(0, 2, 1, 3).reshape(4, 4, 256).max(-1).values - ranges[..., 0])
    assert (deepest[counts > 1024] > 1100).any()
    _fused._state.clear()
    for _ in range(4):   # exact path first, then sync-free; the scene keeps failing its fronts, so the
        img = ms.render_gaussians(*g, cam, background_color=bg, backend="hip")   # lane falls back to full sorts
        assert torch.equal(img, ref)
    if falls_back:
        assert _fused._dev_state(sc["means3d"].device, 0).get("full_sort")
    _fused._state.clear()   # do not leak the fallback into other tests


def test_lazy_front_levels(device, default_grid_only):
    """One heavy 32-px bin (2000 faint specks) whose default sorted front is too short: the lane sees the
    clean-up pass run once and asks for fronts twice as deep -- which hold the whole list -- instead of
    giving up on lazy sorting.  Every frame on the way equals the fully sorted per-stage path."""
    from mojosplat_amd.rasterization import rasterize_gaussians_hip
    from mojosplat_amd.utils import Camera
    gen = torch.Generator().manual_seed(5)
    n, z = 2000, 5.0
    px = 6.0 + 20.0 * torch.rand(n, 2, generator=gen)
    means = torch.cat([(px - 64.0) * z / 60.0, z + 0.5 * torch.rand(n, 1, generator=gen)], 1)
    sc = dict(means3d=means, scales=torch.full((n, 3), -2.3), quats=torch.nn.functional.normalize(torch.randn(n, 4, generator=gen), dim=1),
              opacities=0.005 * (0.9 + 0.2 * torch.rand(n, generator=gen)), features=torch.rand(n, 3, generator=gen))
    sc = {k: v.to(device) for k, v in sc.items()}
    cam = Camera(R=torch.eye(3, device=device), T=torch.zeros(3, device=device), H=128, W=128, fx=60.0, fy=60.0,
                 cx=64.0, cy=64.0)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    m2, con, dep, rad = ms.project_gaussians(*g[:4], cam, backend="hip")
    ids, ranges = ms.bin_gaussians_to_tiles(m2, rad, dep, cam.H, cam.W, 16, backend="hip")
    ref = rasterize_gaussians_hip(m2, con, g[4], g[3], bg, ranges, ids, cam, 16)
    _fused._state.clear()
    levels = []
    for _ in range(5):
        assert torch.equal(ms.render_gaussians(*g, cam, background_color=bg, backend="hip"), ref)
        st = _fused._dev_state(sc["means3d"].device, 0)
        levels.append((st.get("front_level", 0), bool(st.get("full_sort"))))
    assert levels[0] == (0, False) and levels[-1] == (1, False), levels
    _fused._state.clear()


@pytest.mark.parametrize("n,z_hi,opacity", [(4000, 6.0, 0.005), (6000, 4.0, 0.004)])
def test_clean_up_pass_with_fp16_colours(device, default_grid_only, n, z_hi, opacity):
    """The per-bin clean-up kernel of a split frame in its fp16-colour variant (fp32 accumulation as everywhere)."""
    sc, cam = _stack_scene(n, 4.0, z_hi, opacity, device)
    sc["features"] = sc["features"].half()
    bg = torch.tensor(BACKGROUND_V1, device=device)
    ref = stagewise(sc, cam, bg.half(), 16)
    _fused._state.clear()
    for _ in range(3):
        img = ms.render_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"], cam,
                                  background_color=bg.half(), backend="hip")
        assert torch.equal(img, ref)
    _fused._state.clear()


@pytest.mark.parametrize("n,z_lo,z_hi,opacity", [
    (4000, 4.0, 6.0, 0.005),        # one 64-px bin of < 4 096 entries: sorted in LDS in one go
    (16000, 5.0, 5.0, 0.0055),      # ONE depth, 16 000 entries: the sample sort's splitters differ in the index bits alone
    (20000, 4.0, 6.0, 0.0045),      # 20 000 entries over a depth range: splitters, buckets, windows
    (9000, 4.0, 4.0001, 0.0045)])   # a handful of depth values
@pytest.mark.parametrize("px", [64, 32])
def test_two_launch_clean_up_on_coarse_bins(device, n, z_lo, z_hi, opacity, px):
    """Round 4: frames that can expect stranded bins (bins of 48 px and more; any grid once the previous frame redid a
    bin) sort each stranded bin's keys whole in one launch (rasterize.hip, k_redo_sort: LDS bitonic sort up to 4 096
    entries, sample sort beyond) and composite one workgroup per 16x16 block in the next.  The lane is kept on lazily
    sorted fronts (it would go to full sorts after the first failure), so every frame after the first runs the
    clean-up; all must equal the fully sorted per-stage path bit for bit -- fp32 and fp16 colours."""
    sc, cam = _stack_scene(n, z_lo, z_hi, opacity, device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"])
    for feats, bgc in ((sc["features"], bg), (sc["features"].half(), bg.half())):
        ref = stagewise(dict(sc, features=feats), cam, bgc, 16)
        _fused._state.clear()
        _fused.FRAME_STATS = stats = {}
        try:
            for _ in range(5):
                img = ms.render_gaussians(*g, feats, cam, background_color=bgc, backend="hip", bin_size=px)
                assert torch.equal(img, ref)
                st = _fused._dev_state(sc["means3d"].device, 0)
                st["full_sort"] = False
                st["front_level"] = 0
        finally:
            _fused.FRAME_STATS = None
            _fused._state.clear()
        assert stats.get("redo_tiles", 0) >= 2, stats   # (reported one frame late: at least two frames redid their bins)


def test_frames_asked_for_one_call_ahead_equal_blocking_frames(device):
    """render_gaussians(async_op=True): two frames in flight on two lane streams, .wait() one frame later.  Every frame
    equals the blocking call's, through a change of scene and of colour dtype between pending frames, an empty scene
    (zeros, not background) and a consumer on the caller's stream right behind .wait()."""
    bg = torch.tensor(BACKGROUND_V1, device=device)
    scenes = []
    for n, w, h, ell, seed in ((30000, 640, 360, -3.5, 1), (120000, 1280, 720, -4.0, 2), (5000, 333, 205, -3.0, 3)):
        sc, cam = randscene_v1(n, w, h, ell=ell, seed=seed, device=device)
        scenes.append((sc, cam, bg))
    sc16 = dict(scenes[1][0]); sc16["features"] = sc16["features"].half()
    scenes.append((sc16, scenes[1][1], bg.half()))
    far = dict(scenes[0][0]); far["means3d"] = far["means3d"] + torch.tensor([0.0, 0.0, -500.0], device=device)
    scenes.append((far, scenes[0][1], bg))                      # behind the camera: nothing on the grid
    g = lambda s_: (s_["means3d"], s_["scales"], s_["quats"], s_["opacities"], s_["features"])
    _fused._state.clear()
    refs = [ms.render_gaussians(*g(s_), c_, background_color=b_, backend="hip") for s_, c_, b_ in scenes]
    assert float(refs[-1].abs().max()) == 0.0
    order = [0, 1, 0, 3, 1, 4, 2, 2, 3, 0, 4, 1]
    pend, got = None, []
    for k in order:
        s_, c_, b_ = scenes[k]
        nxt = ms.render_gaussians(*g(s_), c_, background_color=b_, backend="hip", async_op=True)
        if pend is not None:
            img = pend[1].wait()
            got.append((pend[0], img, img.sum()))               # (a kernel on the caller's stream right behind the wait)
        pend = (k, nxt)
    img = pend[1].wait()
    got.append((pend[0], img, img.sum()))
    for k, img, total in got:
        assert torch.equal(img, refs[k]), f"scene {k}"
        assert float(total) == float(refs[k].sum())
    with pytest.raises(ValueError):
        ms.render_gaussians(*g(scenes[0][0]), scenes[0][1], backend="torch", async_op=True)
    # release_scratch: refused while a frame is pending on a shared lane, then the scratch goes and frames still render
    s_, c_, b_ = scenes[0]
    pend = ms.render_gaussians(*g(s_), c_, background_color=b_, backend="hip", async_op=True)
    with pytest.raises(RuntimeError):
        ms.release_scratch()
    assert torch.equal(pend.wait(), refs[0])
    ms.release_scratch()
    assert _fused._state.get((sc16["means3d"].device, 0)) is None
    assert torch.equal(ms.render_gaussians(*g(s_), c_, background_color=b_, backend="hip"), refs[0])
    _fused._state.clear()


def test_lane_streams_are_a_calibrated_independent_pair(device):
    """The two streams frames in flight alternate between are chosen once per device by a spin-kernel calibration
    (_fused._lane_streams): distinct streams, neither the caller's, and -- when the calibration ran -- a pair it measured
    as independent (ratio well under the ~1.9 of two streams on one hardware queue)."""
    ls = _fused._lane_streams(device)
    assert len(ls) == 2 and ls[0].cuda_stream != ls[1].cuda_stream
    assert torch.cuda.current_stream(device).cuda_stream not in (ls[0].cuda_stream, ls[1].cuda_stream)
    assert _fused._lane_streams(device) is ls
    rec = _fused.LANE_CALIBRATION.get(device) or _fused.LANE_CALIBRATION.get(torch.device("cuda", torch.cuda.current_device()))
    assert rec is not None
    if rec.get("calibrated"):
        a, b = rec["picked"]
        assert rec["pairs"][f"{a},{b}"] == rec["ratio_of_the_pick"] < 1.6, rec
        assert max(rec["with_current_stream"][a], rec["with_current_stream"][b]) < 1.6, rec


def test_binning_rule_on_a_scene_whose_lane_falls_back_to_full_sorts(device):
    """A pile of faint Gaussians: the lazily sorted split frame fails its fronts and the lane falls back to
    full sorts, while render_gaussians' binning rule (big footprints -> plain coarse bins) moves the grid
    after the first frame.  Every frame on the way is exact, and the rule settles (same mode from the third
    frame on)."""
    from mojosplat_amd import render as R
    sc, cam = _stack_scene(4000, 4.0, 6.0, 0.005, device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    ref = stagewise(sc, cam, bg, 16)
    _fused._state.clear()
    R._bin_mode.clear(); R._bin_left.clear()
    try:
        modes = []
        for _ in range(24):
            assert torch.equal(ms.render_gaussians(*g, cam, background_color=bg, backend="hip"), ref)
            modes.append(next(iter(R._bin_mode.values())))
        assert len(set(modes[2:])) == 1, modes
    finally:
        R._bin_mode.clear(); R._bin_left.clear()
        _fused._state.clear()


@pytest.mark.parametrize("seed", range(10))
def test_fused_path_fuzz_against_stagewise(device, seed):
    """Random scenes through every shortcut of the fused path at once -- tight binning, lazily sorted
    heavy tiles (fixed depth buckets from the camera planes), 1 / 2 / 4 waves per block, sync-free
    repeats, ragged image sizes, near/far planes that cut the cloud -- against the per-stage path
    (gsplat-exact, fully sorted lists, one wave per block with the backward records).  Bit for bit."""
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda lo, hi: lo + (hi - lo) * torch.rand(1, generator=g).item()
    N = int(10 ** r(2.5, 5.2))
    W, H = int(r(40, 700)), int(r(40, 500))
    ell = r(-4.5, -1.5)
    ts = [8, 16, 16, 16, 32][seed % 5]
    sc, cam = randscene_v1(N, W, H, ell=ell, seed=seed, device=device)
    cam.near, cam.far = r(0.05, 4.0), r(6.0, 200.0)
    sc["opacities"] = (sc["opacities"] * r(0.02, 1.0)).clamp(max=1.0)   # faint scenes go deep into their lists
    bg = torch.tensor([r(0, 1), r(0, 1), r(0, 1)], device=device)
    want = stagewise(sc, cam, bg, ts)
    for _ in range(3):
        got = ms.render_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"], cam,
                                  background_color=bg, tile_size=ts, backend="hip")
        assert torch.equal(got, want), (N, W, H, ell, ts)
    _fused._state.clear()


@pytest.mark.parametrize("seed", range(8))
def test_random_row_bands_fuzz_against_stagewise(device, seed):
    """Random scenes cut into random tile-row bands (1-5 of them, any heights: split frames on bands that
    start or end inside a bin row, thin bands on 16-px bins, one-row bands), every band rendered into one
    framebuffer, twice (exact, then sync-free): the per-stage frame, bit for bit."""
    g = torch.Generator().manual_seed(7000 + seed)
    r = lambda lo, hi: lo + (hi - lo) * torch.rand(1, generator=g).item()
    N = int(10 ** r(3.0, 5.3))     # (>= 32 768 Gaussians: bands under 60 % of the rows are pre-culled)
    W, H = int(r(100, 800)), int(r(260, 900))
    sc, cam = randscene_v1(N, W, H, ell=r(-4.0, -2.0), seed=100 + seed, device=device)
    sc["opacities"] = (sc["opacities"] * r(0.05, 1.0)).clamp(max=1.0)
    bg = torch.tensor([r(0, 1), r(0, 1), r(0, 1)], device=device)
    want = stagewise(sc, cam, bg, 16)
    th = -(-H // 16)
    k = 1 + int(r(0, 4.999))
    cuts = sorted({0, th, *[int(r(1, th)) for _ in range(k - 1)]})
    bands = list(zip(cuts[:-1], cuts[1:]))
    args = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    frame = torch.full((H, W, 3), -1.0, device=device)
    # the bands keep their 16-px rows; the bins under them are 16 (split / plain), 32 or 64 px (MS_RENDER_ROWS16)
    ts = [16, 16, 32, 64][seed % 4]
    for _ in range(2):
        for band in bands:
            _fused.render_fwd_hip(*args, cam, bg, ts, row_range=band, out=frame, rows16=True)
        assert torch.equal(frame, want), (N, W, H, bands, ts)
    _fused._state.clear()


def test_fused_path_edge_cases(device):
    """Empty input, a single screen-filling Gaussian (its box exceeds the 64-tile reach mask and is
    walked by whole waves), 1 / 4 / 8 colour channels (lazy sorting only exists for <= 4),
    non-contiguous and strided inputs, fp16 colours -- fused path == per-stage path."""
    bg3 = torch.tensor(BACKGROUND_V1, device=device)
    sc, cam = randscene_v1(3000, 320, 200, ell=-2.5, seed=31, device=device)
    # N = 0 -> zeros image like the reference (render.py:73-76)
    z = ms.render_gaussians(sc["means3d"][:0], sc["scales"][:0], sc["quats"][:0], sc["opacities"][:0],
                            sc["features"][:0], cam, background_color=bg3, backend="hip")
    assert z.shape == (200, 320, 3) and (z == 0).all()
    # one Gaussian covering the whole image, plus the cloud behind it
    big = dict(means3d=torch.cat([torch.tensor([[0.0, 0.0, 2.0]], device=device), sc["means3d"]]),
               scales=torch.cat([torch.full((1, 3), 1.0, device=device), sc["scales"]]),
               quats=torch.cat([torch.tensor([[1.0, 0, 0, 0]], device=device), sc["quats"]]),
               opacities=torch.cat([torch.tensor([0.3], device=device), sc["opacities"]]),
               features=torch.cat([torch.tensor([[0.9, 0.1, 0.2]], device=device), sc["features"]]))
    a = ms.render_gaussians(big["means3d"], big["scales"], big["quats"], big["opacities"], big["features"], cam,
                            background_color=bg3, backend="hip")
    assert torch.equal(a, stagewise(big, cam, bg3, 16))
    # channel counts
    for C in (1, 4, 8):
        scC = dict(sc, features=torch.rand(3000, C, generator=torch.Generator().manual_seed(C)).to(device))
        bgC = torch.linspace(0.1, 0.6, C, device=device)
        a = ms.render_gaussians(scC["means3d"], scC["scales"], scC["quats"], scC["opacities"], scC["features"], cam,
                                background_color=bgC, backend="hip")
        assert a.shape == (200, 320, C) and torch.equal(a, stagewise(scC, cam, bgC, 16))
    # strided views of bigger tensors
    pad = {k: torch.cat([v, v], dim=-1) if v.dim() > 1 else torch.stack([v, v], 1) for k, v in sc.items()}
    view = dict(means3d=pad["means3d"][:, :3], scales=pad["scales"][:, 3:], quats=pad["quats"][:, 4:],
                opacities=pad["opacities"][:, 1], features=pad["features"][:, :3])
    assert not view["means3d"].is_contiguous()
    assert torch.equal(ms.render_gaussians(view["means3d"], view["scales"], view["quats"], view["opacities"],
                                           view["features"], cam, background_color=bg3, backend="hip"),
                       stagewise(sc, cam, bg3, 16))


@pytest.mark.parametrize("world", [2, 3, 8])
def test_sharded_rehearsal_assembles_the_frame(device, world):
    """Every rank's share of a frame through the asynchronous sharded entry point (lane streams,
    split-phase, band-only tile scan, lazily sorted band lists), without a process group: the
    slabs put together equal the single-GPU frame; two frames in flight per 'rank'."""
    from mojosplat_amd.distributed import band_plan, render_gaussians_sharded
    sc, cam = randscene_v1(40_000, 640, 360, ell=-2.8, seed=23, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    ref = ms.render_gaussians(*g, cam, background_color=bg, backend="hip")
    th = -(-cam.H // 16)
    rows, bands = band_plan(th, world)
    out = torch.zeros_like(ref)
    for r, (r0, r1) in enumerate(bands):
        a = render_gaussians_sharded(*g, cam, background_color=bg, async_op=True, rehearse=(r, world))
        b = render_gaussians_sharded(*g, cam, background_color=bg, async_op=True, rehearse=(r, world))
        ia, ib = a.wait(), b.wait()
        y0, y1 = r0 * 16, min(r1 * 16, cam.H)
        assert torch.equal(ia[y0:y1], ib[y0:y1])
        out[y0:y1] = ia[y0:y1]
    assert torch.equal(out, ref)


def test_frame_does_not_depend_on_the_binning_granularity(device):
    """A pixel blends the same Gaussians in the same order whatever tile grid they were binned on, so
    16 / 32 / 64-px bins (the rasteriser works in 16x16 blocks inside any tile) give the same frame bit
    for bit -- which is what lets render_gaussians pick the fastest grid for a scene on its own."""
    from mojosplat_amd import render as R
    sc, cam = randscene_v1(60_000, 512, 384, ell=-2.6, seed=41, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    ref = stagewise(sc, cam, bg, 16)
    for ts in (16, 32, 64):
        _fused._state.clear()
        for _ in range(2):
            assert torch.equal(ms.render_gaussians(*g, cam, background_color=bg, tile_size=ts, backend="hip"), ref), ts
    # explicit bin sizes, and the automatic choice (a rule on the previous frame's record): same pixels
    for b in (16, 32, 64):
        _fused._state.clear()
        for _ in range(2):
            assert torch.equal(ms.render_gaussians(*g, cam, background_color=bg, bin_size=b, backend="hip"), ref), b
    with pytest.raises(ValueError, match="bin_size"):
        ms.render_gaussians(*g, cam, background_color=bg, bin_size=48, backend="hip")
    _fused._state.clear()
    R._bin_mode.clear(); R._bin_left.clear()
    try:
        seen = set()
        for _ in range(6):
            assert torch.equal(ms.render_gaussians(*g, cam, background_color=bg, backend="hip"), ref)
            seen.add(next(iter(R._bin_mode.values())))
        assert len(R._bin_mode) == 1 and seen <= {16, 32, 64}
        best, times = R.tune_binning(*g, cam, background_color=bg, frames=2)   # the opt-in measurement
        assert best in (16, 32, 64) and set(times) == {16, 32, 64} and all(t > 0 for t in times.values())
    finally:
        R._bin_mode.clear(); R._bin_left.clear()
        _fused._state.clear()


def test_bands_of_16px_rows_under_coarse_bins(device):
    """MS_RENDER_ROWS16: a multi-GPU rank's band keeps its 16-px rows while the bins are 32 or 64 px (dense
    scenes): the band is binned on the tile rows that cover it and rasterised on exactly its rows.  Bands cut
    anywhere assemble to the full frame bit for bit, and nothing outside a band's rows is written."""
    sc, cam = randscene_v1(60_000, 512, 384, ell=-2.6, seed=41, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    ref = stagewise(sc, cam, bg, 16)
    th = 384 // 16
    for ts in (32, 64):
        for cuts in ((0, 5, 6, 13, th), (0, 1, th - 1, th), (0, 9, 9, 18, th)):
            frame = torch.full_like(ref, -7.0)
            for r0, r1 in zip(cuts[:-1], cuts[1:]):
                before = frame.clone()
                _fused.render_fwd_hip(*g, cam, bg, ts, row_range=(r0, r1), out=frame, rows16=True)
                keep = torch.ones(384, dtype=torch.bool, device=device)
                keep[r0 * 16:r1 * 16] = False
                assert torch.equal(frame[keep], before[keep]), (ts, r0, r1)   # only the band's rows were touched
            assert torch.equal(frame, ref), (ts, cuts)


def test_split_frame_restarts_on_16px_tiles_when_its_bins_hold_too_much(device):
    """A split frame whose 32-px bins hold more entries than 4 block-list slots each can index (2^29;
    lowered to 1000 through the environment here, in a fresh process since the library reads it once)
    is started again on 16-px tiles -- also across the grow-the-buffer redo -- and gives the same frame."""
    import os, subprocess, sys
    code = """
import torch, mojosplat_amd as ms
from mojosplat_amd import _fused
from mojosplat_amd.scenes import BACKGROUND_V1, randscene_v1
dev = torch.device("cuda", 0)
sc, cam = randscene_v1(30000, 480, 320, ell=-2.8, seed=77, device=dev)
bg = torch.tensor(BACKGROUND_V1, device=dev)
g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
m2, con, dep, rad = ms.project_gaussians(*g[:4], cam, backend="hip")
ids, ranges = ms.bin_gaussians_to_tiles(m2, rad, dep, cam.H, cam.W, 16, backend="hip")
ref = ms.rasterize_gaussians(m2, con, g[4], g[3], bg, ranges, ids, cam, tile_size=16, backend="hip")
for i in range(4):
    img, m = _fused.render_fwd_hip(*g, cam, bg, 16)
    assert torch.equal(img, ref), i
    assert m > 1000 and int(_fused._dev_state(dev, 0)["host"][7]) & 16, (i, m)
print("OK")
"""
    env = dict(os.environ, MOJOSPLAT_SPLIT_MAX_ENTRIES="1000")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


def test_light_frame_bet_is_repaired_when_heavy_tiles_appear(device):
    """A frame whose predecessor (same scratch, same grid) had no list beyond the small sort class only launches
    the small sorts (ms_render_fwd bets on it, bit 5 of the size record's flag word).  When the next scene DOES
    hold heavy tiles -- the same number of Gaussians, fewer pairs, all in a few bins, so the intersection buffer
    still fits and nothing else sends the frame to the exact path -- the bet fails, the frame is redone, and
    the image is still the per-stage path's, bit for bit."""
    _fused._state.clear()
    N, W, H = 10_000, 640, 360
    bg = torch.tensor(BACKGROUND_V1, device=device)
    sc, cam = randscene_v1(N, W, H, ell=-3.5, seed=5, device=device)
    args = lambda s: (s["means3d"], s["scales"], s["quats"], s["opacities"], s["features"])
    for _ in range(3):   # settle on a grid; the last of these frames runs on the bet
        a = ms.render_gaussians(*args(sc), cam, background_color=bg, bin_size=32)
    st = _fused._dev_state(device, 0)
    assert int(st["host_np"][2]) + int(st["host_np"][3]) + int(st["host_np"][4]) == 0, "the light scene must hold no heavy bin"
    assert int(st["host_np"][7]) & 32, "the frame after a light frame runs on the bet"
    assert torch.equal(a, stagewise(sc, cam, bg))
    m_light = int(st["host_np"][0])
    # the same Gaussians pulled towards the view axis and shrunk: fewer pairs, a few crowded bins
    dense = dict(sc)
    dense["means3d"] = sc["means3d"] * torch.tensor([0.12, 0.12, 1.0], device=device)
    dense["scales"] = sc["scales"] - 1.2
    b = ms.render_gaussians(*args(dense), cam, background_color=bg, bin_size=32)
    heavy = int(st["host_np"][2]) + int(st["host_np"][3]) + int(st["host_np"][4])
    assert heavy > 0 and int(st["host_np"][0]) <= 1.2 * m_light, (heavy, int(st["host_np"][0]), m_light)
    assert int(st["host_np"][7]) & 4, "the failed bet sends the frame to the exact path"
    assert torch.equal(b, stagewise(dense, cam, bg))
    # and the frame after it (its predecessor had heavy bins) does not bet
    b2 = ms.render_gaussians(*args(dense), cam, background_color=bg, bin_size=32)
    assert not (int(st["host_np"][7]) & 32) and torch.equal(b, b2)


def _orbit(cam, angle):
    import math
    from mojosplat_amd.utils import Camera
    c, s = math.cos(angle), math.sin(angle)
    ry = torch.tensor([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], device=cam.R.device)
    return Camera(R=cam.R @ ry, T=cam.T, H=cam.H, W=cam.W, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)


@pytest.mark.parametrize("N,W,H,ell,px", [(500_000, 1280, 720, -3.5, 32), (500_000, 1280, 720, -3.0, 64)])
def test_depth_cut_frames_equal_uncut_frames(device, monkeypatch, N, W, H, ell, px):
    """Sync-free frames on plain bins drop the pairs behind the depth at which the previous frame's sorted front of
    their bin ended (csrc/binning.hip, k_project_hist; forced here whatever the scene's size: MOJOSPLAT_DEPTH_CUT=2).
    Bit for bit the uncut frames (MOJOSPLAT_DEPTH_CUT=0): on a still camera, along an orbit, and across a swap to a scene
    whose near Gaussians have all but vanished -- stale cut-offs that leave bins short of pairs, which the clean-up
    launches regenerate from the box records (rasterize.hip, k_far_regen) -- and back.  "denser": the same Gaussians
    at twice the size, three to four times the pairs on the same grid and scratch -- a frame that starts with the cut
    outgrows the intersection buffer and is started over without it."""
    bg = torch.tensor(BACKGROUND_V1, device=device)
    sc, cam = randscene_v1(N, W, H, ell=ell, seed=42, device=device)   # (a scene whose sorted fronts saturate its pixels)
    faint = dict(sc)
    depth = (sc["means3d"] @ cam.R.T + cam.T)[:, 2]
    faint["opacities"] = torch.where(depth < depth.median(), sc["opacities"] * 0.02, sc["opacities"])
    sequences = {
        "still": [(sc, cam)] * 5,
        "orbit": [(sc, _orbit(cam, 0.004 * i)) for i in range(8)],
        "swap": [(sc, cam)] * 3 + [(faint, cam)] * 3 + [(sc, cam)] * 2,
    }
    if px == 32:   # a larger scene on the same grid: the lane's scratch is reallocated, its cut-offs with it
        big, _ = randscene_v1(N + N // 2, W, H, ell=ell, seed=43, device=device)
        sequences["grow"] = [(sc, cam)] * 3 + [(big, cam)] * 4
        denser = dict(sc)
        denser["scales"] = sc["scales"] + math.log(2.0)
        sequences["denser"] = [(sc, cam)] * 3 + [(denser, cam)] * 2

    def run(mode, seq):
        _hip_mod.config_depth_cut(int(mode))
        _fused._state.clear()
        _fused.FRAME_STATS = {}
        try:
            frames = [ms.render_gaussians(s["means3d"], s["scales"], s["quats"], s["opacities"], s["features"], c,
                                          background_color=bg, bin_size=px).clone() for s, c in seq]
            torch.cuda.synchronize()
            return frames, dict(_fused.FRAME_STATS)
        finally:
            _fused.FRAME_STATS = None

    for label, seq in sequences.items():
        ref, st0 = run("0", seq)
        got, st = run("2", seq)
        # (the faint scene's fronts do not saturate its pixels either: the lane ends up on full sorts, which take no cut)
        assert st0.get("depth_cut", 0) == 0 and st.get("depth_cut", 0) >= (len(seq) - 4 if label in ("still", "orbit") else 1), (label, st)
        for k, (a, b) in enumerate(zip(ref, got)):
            assert torch.equal(a, b), (label, k, float((a - b).abs().max()))
        assert st.get("regen_mismatch", 0) == 0, (label, st)   # the clean-up launches and the count kernel agree on every pair
        if label in ("still", "orbit"):
            assert st.get("cut_redo_tiles", 0) == 0, (label, st)   # the cut-offs hold while the view changes slowly
        elif label == "swap":
            assert st.get("cut_redo_tiles", 0) > 0, st                # ... and the swap is what the fallback is for
        elif label == "denser":
            # (the frames before the denser ones took the cut -- the count above -- and left the record a cut frame starts
            # from; the first denser frame overflowed a buffer grown with 1.25 slack for a third of its pairs)
            assert st.get("overflow", 0) >= 1, st
    # the first frame of a sequence is the per-stage path's (an uncut frame of the fused path is tested to be)
    assert torch.equal(ref[0], stagewise(sc, cam, bg, 16))
    _fused._state.clear()


@pytest.mark.parametrize("px,world", [(32, 4), (64, 3), (32, 8)])
def test_depth_cut_on_band_frames(device, px, world):
    """Round 4: a rank's band of a frame takes the depth cut too -- cut-offs kept per band (rows and 16-px clip in the size
    record's signature), the count kernel's deferred records and the regeneration launches working on POSITIONS of the
    band's pre-culled candidate list.  Every band's frames with the cut forced equal its frames without, bit for bit --
    still camera, orbit, and a swap to a scene whose near half has all but vanished (stale cut-offs: bins get their pairs
    back from k_far_regen by position) -- and the bands of the first frame assemble the per-stage path's image.  The last
    two frames hold the same Gaussians at twice the size: a band's cut frame that outgrows its intersection buffer is
    started over without the cut, its rows handed back in the units the caller gave them.  (Three more frames of the scene
    come before them: the swap leaves the lane on full sorts for four frames, which take no cut and leave no cut-offs.)"""
    from mojosplat_amd.distributed import band_plan
    N, W, H, ell = 400_000, 1280, 720, (-3.5 if px != 64 else -3.0)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    sc, cam = randscene_v1(N, W, H, ell=ell, seed=42, device=device)
    faint = dict(sc)
    depth = (sc["means3d"] @ cam.R.T + cam.T)[:, 2]
    faint["opacities"] = torch.where(depth < depth.median(), sc["opacities"] * 0.02, sc["opacities"])
    denser = dict(sc)
    denser["scales"] = sc["scales"] + math.log(2.0)
    seq = [(sc, cam)] * 4 + [(sc, _orbit(cam, 0.004 * i)) for i in range(1, 5)] + [(faint, cam)] * 3 + [(sc, cam)] * 5 + [(denser, cam)] * 2
    th16 = -(-H // 16)
    _, bands = band_plan(th16, world)
    ref0 = stagewise(sc, cam, bg, 16)
    assembled = torch.zeros_like(ref0)
    totals, primed = {}, 0
    try:
        for r0, r1 in bands:
            y0, y1 = r0 * 16, min(r1 * 16, H)

            def run(mode):
                _hip_mod.config_depth_cut(int(mode))
                _fused._state.clear()
                _fused.FRAME_STATS = st = {}
                frames, culled, flags = [], 0, []
                for s_, c_ in seq:
                    buf = torch.zeros((H, W, 3), device=device)
                    info = {}
                    _fused.render_fwd_hip(s_["means3d"], s_["scales"], s_["quats"], s_["opacities"], s_["features"], c_, bg, px,
                                          row_range=(r0, r1), out=buf, info=info, rows16=(px != 16))
                    culled += 1 if info["flags"] & 2048 else 0
                    flags.append(info["flags"])
                    frames.append(buf[y0:y1].clone())
                torch.cuda.synchronize()
                _fused.FRAME_STATS = None
                return frames, st, culled, flags
            ref, st0, _, _ = run(0)
            got, st, culled, flags = run(2)
            # (bits 6 and 7 of the flag word: the frame took the cut and left cut-offs -- the next frame starts as a cut frame)
            primed += 1 if (flags[-3] & 64) and (flags[-3] & 128) else 0
            assert st0.get("depth_cut", 0) == 0, (r0, r1, st0)   # (a sparse edge band has no heavy bin and takes no cut: the total below)
            assert culled == len(seq), "the bands of this test are pre-culled"
            assert st.get("regen_mismatch", 0) == 0, st
            for k, (a, b) in enumerate(zip(ref, got)):
                assert torch.equal(a, b), ((r0, r1), k, float((a - b).abs().max()))
            assembled[y0:y1] = got[0]
            for k_, v_ in st.items():
                totals[k_] = totals.get(k_, 0) + v_
    finally:
        _fused.FRAME_STATS = None
        _fused._state.clear()
    assert torch.equal(assembled, ref0)
    assert totals.get("depth_cut", 0) >= 4 * (world // 2), totals   # at least the centre bands cut most of their frames
    assert totals.get("cut_redo_tiles", 0) > 0, totals   # the swap did strand bins whose cut-offs were stale
    assert primed >= 1, "the frame before the denser ones took the cut in no band"
    assert totals.get("overflow", 0) >= 1, totals   # the denser frames outgrew a buffer sized with 1.25 slack for a third of their pairs


@pytest.mark.parametrize("seed", range(6))
def test_depth_cut_fuzz_against_stagewise(device, monkeypatch, seed, dense=False):
    """Random scenes, image sizes, plain bin sizes, near / far planes and opacity scales, from a camera that drifts a
    little every frame, with the depth cut forced on every frame that can take it: every frame equals the per-stage
    path (fully sorted gsplat-exact lists) bit for bit -- whether its cut-offs held, bins got their pairs back from the
    clean-up launches, or the lane gave up on lazily sorted fronts altogether."""
    import math
    from mojosplat_amd.utils import Camera
    _hip_mod.config_depth_cut(2)
    g = torch.Generator().manual_seed(31000 + seed)
    r = lambda lo, hi: lo + (hi - lo) * torch.rand(1, generator=g).item()
    if dense:   # (scripts/fuzz_cut.py: scenes whose fronts saturate their pixels, so that most frames do take the cut)
        N, W, H, ell = int(10 ** r(5.4, 6.0)), int(r(1000, 1920)), int(r(600, 1080)), r(-3.8, -3.0)
    else:
        N, W, H, ell = int(10 ** r(4.3, 5.6)), int(r(300, 1400)), int(r(200, 900)), r(-4.2, -2.8)
    px = [32, 64][seed % 2]
    sc, cam = randscene_v1(N, W, H, ell=ell, seed=900 + seed, device=device)
    cam.near, cam.far = r(0.05, 2.0), r(8.0, 200.0)
    sc["opacities"] = (sc["opacities"] * r(0.7 if dense else 0.3, 1.0)).clamp(max=1.0)
    bg = torch.tensor([r(0, 1), r(0, 1), r(0, 1)], device=device)
    args = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    _fused._state.clear()
    _fused.FRAME_STATS = {}
    try:
        for k in range(7):
            a = 0.01 * k * (1 if seed % 3 else -1)
            c, s = math.cos(a), math.sin(a)
            ry = torch.tensor([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], device=device)
            cm = Camera(R=cam.R @ ry, T=cam.T + torch.tensor([0.0, 0.0, 0.02 * k], device=device), H=H, W=W, fx=cam.fx, fy=cam.fy,
                        cx=cam.cx, cy=cam.cy, near=cam.near, far=cam.far)
            got = ms.render_gaussians(*args, cm, background_color=bg, bin_size=px)
            want = stagewise(sc, cm, bg, 16)
            assert torch.equal(got, want), (seed, k, N, W, H, px, dict(_fused.FRAME_STATS), float((got - want).abs().max()))
    finally:
        LAST_CUT_FUZZ_STATS.clear()
        LAST_CUT_FUZZ_STATS.update(_fused.FRAME_STATS or {})
        _fused.FRAME_STATS = None
        _fused._state.clear()


@pytest.mark.parametrize("seed", range(6))
def test_band_depth_cut_fuzz_against_stagewise(device, seed, dense=False):
    """The depth-cut fuzz on a rank's BAND of the frame: a random run of 16-px rows (pre-culled when it is under 60 % of
    the image and the scene is large enough), bins of 32 or 64 px under it, a camera that drifts every frame and a swap to
    the same Gaussians with the near half nearly transparent half-way -- stale cut-offs, bins regenerated by POSITION in
    the band's candidate list.  The band's rows of every frame equal the per-stage path's, bit for bit, and nothing is
    written outside them."""
    import math
    from mojosplat_amd.utils import Camera
    _hip_mod.config_depth_cut(2)
    g = torch.Generator().manual_seed(47000 + seed)
    r = lambda lo, hi: lo + (hi - lo) * torch.rand(1, generator=g).item()
    if dense:
        N, W, H, ell = int(10 ** r(5.3, 5.9)), int(r(1000, 1920)), int(r(600, 1080)), r(-3.8, -3.0)
    else:
        N, W, H, ell = int(10 ** r(4.4, 5.5)), int(r(400, 1400)), int(r(300, 900)), r(-4.0, -2.8)
    px = [32, 64][seed % 2]
    sc, cam = randscene_v1(N, W, H, ell=ell, seed=1900 + seed, device=device)
    sc["opacities"] = (sc["opacities"] * r(0.7 if dense else 0.4, 1.0)).clamp(max=1.0)
    faint = dict(sc)
    depth = (sc["means3d"] @ cam.R.T + cam.T)[:, 2]
    faint["opacities"] = torch.where(depth < depth.median(), sc["opacities"] * 0.03, sc["opacities"])
    bg = torch.tensor([r(0, 1), r(0, 1), r(0, 1)], device=device)
    th = -(-H // 16)
    r0 = int(r(0, th - 1))
    r1 = min(th, r0 + 1 + int(r(0, max(1.0, 0.7 * th))))
    y0, y1 = r0 * 16, min(r1 * 16, H)
    _fused._state.clear()
    _fused.FRAME_STATS = {}
    try:
        for k in range(9):
            a = 0.008 * k * (1 if seed % 3 else -1)
            c, s = math.cos(a), math.sin(a)
            ry = torch.tensor([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], device=device)
            cm = Camera(R=cam.R @ ry, T=cam.T + torch.tensor([0.0, 0.0, 0.015 * k], device=device), H=H, W=W, fx=cam.fx, fy=cam.fy,
                        cx=cam.cx, cy=cam.cy, near=cam.near, far=cam.far)
            s_ = faint if 4 <= k < 7 else sc
            frame = torch.full((H, W, 3), -1.0, device=device)
            _fused.render_fwd_hip(s_["means3d"], s_["scales"], s_["quats"], s_["opacities"], s_["features"], cm, bg, px,
                                  row_range=(r0, r1), out=frame, rows16=True)
            want = stagewise(s_, cm, bg, 16)
            what = (seed, k, N, W, H, px, (r0, r1), dict(_fused.FRAME_STATS))
            assert torch.equal(frame[y0:y1], want[y0:y1]), what + (float((frame[y0:y1] - want[y0:y1]).abs().max()),)
            assert bool((frame[:y0] == -1.0).all()) and bool((frame[y1:] == -1.0).all()), what
            assert _fused.FRAME_STATS.get("regen_mismatch", 0) == 0, what
    finally:
        LAST_CUT_FUZZ_STATS.clear()
        LAST_CUT_FUZZ_STATS.update(_fused.FRAME_STATS or {})
        _fused.FRAME_STATS = None
        _fused._state.clear()


LAST_CUT_FUZZ_STATS = {}   # (scripts/fuzz_cut.py sums these up: how many frames took the cut, how many bins were regenerated)


def test_a_lane_on_full_sorts_tries_lazy_sorting_again(device, default_grid_only, monkeypatch):
    """A lane whose lazily sorted fronts kept failing sorts fully -- but not for ever: after RETRY_FULL_SORT frames it
    tries fronts again (here 2 frames, on a scene that fails them every time: back to full sorts with twice the patience),
    and a scene that has become opaque again stays on the fast path.  Every frame equals the per-stage path."""
    from mojosplat_amd.rasterization import rasterize_gaussians_hip
    monkeypatch.setattr(_fused, "RETRY_FULL_SORT", 2)
    bg = torch.tensor(BACKGROUND_V1, device=device)

    def reference(sc, cam):
        g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
        m2, con, dep, rad = ms.project_gaussians(*g[:4], cam, backend="hip")
        ids, ranges = ms.bin_gaussians_to_tiles(m2, rad, dep, cam.H, cam.W, 16, backend="hip")
        return g, rasterize_gaussians_hip(m2, con, g[4], g[3], bg, ranges, ids, cam, 16)

    faint, cam = _stack_scene(4000, 4.0, 6.0, 0.005, device)
    solid = dict(faint)
    solid["opacities"] = torch.full_like(faint["opacities"], 0.9)
    solid["scales"] = faint["scales"] + 2.0   # (wide enough for the corner pixels to saturate within a front as well)
    (gf, ref_f), (gs, ref_s) = reference(faint, cam), reference(solid, cam)
    _fused._state.clear()
    _fused.FRAME_STATS = {}
    try:
        modes = []
        for k in range(12):
            assert torch.equal(ms.render_gaussians(*gf, cam, background_color=bg, backend="hip"), ref_f), k
            modes.append(bool(_fused._dev_state(device, 0).get("full_sort")))
        st = dict(_fused.FRAME_STATS)
        assert st.get("full_sort_on", 0) >= 2 and st.get("lazy_sort_retry", 0) >= 2, (st, modes)
        assert _fused._dev_state(device, 0).get("retry_after", 0) >= 8, _fused._dev_state(device, 0).get("retry_after")
        left = None
        for k in range(80):   # the fog lifts: the next retry (within the patience reached above: <= 64 frames) sticks
            assert torch.equal(ms.render_gaussians(*gs, cam, background_color=bg, backend="hip"), ref_s), k
            if left is None and not _fused._dev_state(device, 0).get("full_sort"):
                left = k
        assert left is not None and not _fused._dev_state(device, 0).get("full_sort"), (left, _fused._dev_state(device, 0).get("retry_after"))
    finally:
        _fused.FRAME_STATS = None
        _fused._state.clear()


def test_prepared_scene_bands_equal_the_single_gpu_frame(device):
    """Round 5: a PREPARED scene (scene_order.prepare_scene: Morton order + the bounds of every block of 256 Gaussians) through
    the sharded entry point -- the band pre-cull skips whole blocks by their bounds.  Every rank's band (8 and 3 ranks,
    blocking and two frames in flight, a moved camera, bands that hold nothing) assembles to the single-GPU frame of the SAME
    arrays bit for bit, the candidates the library reports are never more than without the bounds would give, and a scene
    whose tensors were modified in place after prepare_scene silently loses its bounds instead of culling with stale ones."""
    from mojosplat_amd.distributed import render_gaussians_sharded
    from mojosplat_amd.scene_order import prepare_scene, prepared_bounds
    from mojosplat_amd.utils import Camera
    sc, cam = randscene_v1(200_000, 1280, 720, ell=-3.6, seed=11, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    ps = prepare_scene(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
    g = ps.arrays
    assert prepared_bounds(g[0], g[1]) is not None and ps.block_bounds.shape == (-(-200_000 // 256), 8)
    # the bounds hold: every Gaussian inside its block's box, its largest scale under the block's
    blk = torch.arange(200_000, device=device) // 256
    lo, hi, sm = ps.block_bounds[blk, 0:3], ps.block_bounds[blk, 4:7], ps.block_bounds[blk, 3]
    assert bool((g[0] >= lo).all()) and bool((g[0] <= hi).all()) and bool((g[1].exp().max(1).values <= sm).all())
    th = -(-cam.H // 16)
    cams = [cam]
    c, s_ = math.cos(0.4), math.sin(0.4)
    R2 = torch.tensor([[c, 0.0, s_], [0.0, 1.0, 0.0], [-s_, 0.0, c]], device=device) @ cam.R
    cams.append(Camera(R=R2.contiguous(), T=cam.T + torch.tensor([0.3, -0.2, -2.0], device=device), H=cam.H, W=cam.W, fx=cam.fx,
                       fy=cam.fy, cx=cam.cx, cy=cam.cy, near=cam.near, far=cam.far))   # (closer: boxes straddle the near plane)
    for cm in cams:
        ref = ms.render_gaussians(*g, cm, background_color=bg, backend="hip")
        same = ms.render_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"], cm, background_color=bg)
        # (a permutation moves the order of Gaussians at bit-equal depth -- ties go by index -- and nothing else: a few
        # pixels under such a pair change by up to an alpha, the rest of the frame is the same to the bit)
        d = (ref - same).abs().max(-1).values
        assert float((d > 0).float().mean()) <= 1e-3 and float(d.max()) <= 0.05
        for world in (8, 3):
            frame = torch.empty_like(ref)
            rows = -(-th // world)
            for r in range(world):
                band = render_gaussians_sharded(*g, cm, background_color=bg, rehearse=(r, world))
                y0, y1 = min(r * rows * 16, cm.H), min((r + 1) * rows * 16, cm.H)
                frame[y0:y1] = band[y0:y1]
            assert torch.equal(frame, ref), f"world {world}: the prepared scene's bands differ from the single-GPU frame"
        # two frames in flight on the lane streams
        cur = None
        for k in range(5):
            nxt = render_gaussians_sharded(*g, cm, background_color=bg, rehearse=(3, 8), async_op=True)
            if cur is not None:
                b = cur.wait()
                y0, y1 = 3 * (-(-th // 8)) * 16, min(4 * (-(-th // 8)) * 16, cm.H)
                assert torch.equal(b[y0:y1], ref[y0:y1])
            cur = nxt
        cur.wait()
    # an in-place update of the means voids the bounds (their box no longer holds): the scene renders as an unprepared one
    g[0].add_(0.5)
    assert prepared_bounds(g[0], g[1]) is None
    ref = ms.render_gaussians(*g, cam, background_color=bg, backend="hip")
    frame = torch.empty_like(ref)
    rows = -(-th // 8)
    for r in range(8):
        band = render_gaussians_sharded(*g, cam, background_color=bg, rehearse=(r, 8))
        y0, y1 = min(r * rows * 16, cam.H), min((r + 1) * rows * 16, cam.H)
        frame[y0:y1] = band[y0:y1]
    assert torch.equal(frame, ref)


@pytest.mark.parametrize("world,rank", [(4, 1), (8, 4), (3, 0)])
def test_band_pair_defers_its_clean_up_to_the_finishing_half(device, monkeypatch, world, rank):
    """Round 5: a band in flight behind another (two lanes, ms_render_band_begin / _finish) does not enqueue the clean-up
    launches -- up to four, empty on almost every frame -- behind its rasteriser (MS_RENDER_DEFER_CLEANUP): the finishing half
    waits for the band's end, reads the rasteriser's verdict from the lane's pinned record and enqueues them only when a bin
    asked for them.  Depth cuts forced, a still camera, an orbit and a swap to a scene whose near half has all but vanished
    (stale cut-offs: stranded bins, the clean-up IS needed): every pipelined band equals the single-GPU frame's rows bit for
    bit, with the deferral and without it (MOJOSPLAT_DEFER_CLEANUP=0), and the deferred run did enqueue clean-ups late."""
    from mojosplat_amd.distributed import render_gaussians_sharded
    N, W, H = 400_000, 1280, 720
    bg = torch.tensor(BACKGROUND_V1, device=device)
    sc, cam = randscene_v1(N, W, H, ell=-3.5, seed=42, device=device)
    faint = dict(sc)
    depth = (sc["means3d"] @ cam.R.T + cam.T)[:, 2]
    faint["opacities"] = torch.where(depth < depth.median(), sc["opacities"] * 0.02, sc["opacities"])
    seq = [(sc, cam)] * 5 + [(sc, _orbit(cam, 0.004 * i)) for i in range(1, 5)] + [(faint, cam)] * 4 + [(sc, cam)] * 3
    arrays = lambda s_: (s_["means3d"], s_["scales"], s_["quats"], s_["opacities"], s_["features"])
    _hip_mod.config_depth_cut(0)
    refs = [ms.render_gaussians(*arrays(s_), c_, background_color=bg, backend="hip") for s_, c_ in seq]
    th = -(-H // 16)
    rows = -(-th // world)
    y0, y1 = min(rank * rows * 16, H), min((rank + 1) * rows * 16, H)
    results = {}
    try:
        for defer in ("0", "1"):
            monkeypatch.setenv("MOJOSPLAT_DEFER_CLEANUP", defer)
            _hip_mod.config_depth_cut(2)
            _fused._state.clear()
            _fused.FRAME_STATS = st = {}
            cur, k_cur = None, -1
            for k, (s_, c_) in enumerate(seq):
                nxt = render_gaussians_sharded(*arrays(s_), c_, background_color=bg, rehearse=(rank, world), async_op=True)
                if cur is not None:
                    b = cur.wait()
                    assert torch.equal(b[y0:y1], refs[k_cur][y0:y1]), (defer, k_cur, float((b[y0:y1] - refs[k_cur][y0:y1]).abs().max()))
                cur, k_cur = nxt, k
            b = cur.wait()
            assert torch.equal(b[y0:y1], refs[k_cur][y0:y1]), (defer, k_cur)
            torch.cuda.synchronize()
            results[defer] = dict(st)
    finally:
        _fused.FRAME_STATS = None
        _fused._state.clear()
    off, on = results["0"], results["1"]
    assert off.get("cleanup_deferred", 0) == 0, off
    assert on.get("cleanup_deferred", 0) >= len(seq) // 2, on          # most frames ran sync-free with the clean-up left out
    assert on.get("cleanup_enqueued_late", 0) > 0, on                   # ... and the swap's frames asked for it after all
    assert on.get("cleanup_enqueued_late", 0) < on["cleanup_deferred"], on   # (quiet frames enqueue nothing)
    assert on.get("regen_mismatch", 0) == 0 and off.get("regen_mismatch", 0) == 0


@pytest.mark.parametrize("seed", range(6))
def test_pipelined_band_fuzz_with_deferred_clean_up(device, seed, dense=False):
    """Random scenes, image sizes, world sizes and ranks through the ASYNCHRONOUS sharded entry point (two lanes, the band pair
    with its clean-up launches left to the finishing half), depth cuts forced, a camera that drifts every frame, a swap to the
    same Gaussians with the near half nearly transparent half-way and back: the band's rows of every frame equal the
    single-GPU frame's bit for bit, in float32 and -- every other seed -- through a float16 exchange (the rounded rows)."""
    import math
    from mojosplat_amd.distributed import band_plan, render_gaussians_sharded
    from mojosplat_amd.utils import Camera
    g = torch.Generator().manual_seed(91000 + seed)
    r = lambda lo, hi: lo + (hi - lo) * torch.rand(1, generator=g).item()
    if dense:
        N, W, H, ell = int(10 ** r(5.3, 5.9)), int(r(1000, 1920)), int(r(600, 1080)), r(-3.8, -3.0)
    else:
        N, W, H, ell = int(10 ** r(4.6, 5.6)), int(r(500, 1500)), int(r(300, 900)), r(-4.0, -2.8)
    world = [2, 3, 4, 8][seed % 4]
    rank = int(r(0, world - 1e-3))
    sc, cam = randscene_v1(N, W, H, ell=ell, seed=2300 + seed, device=device)
    sc["opacities"] = (sc["opacities"] * r(0.5, 1.0)).clamp(max=1.0)
    faint = dict(sc)
    depth = (sc["means3d"] @ cam.R.T + cam.T)[:, 2]
    faint["opacities"] = torch.where(depth < depth.median(), sc["opacities"] * 0.03, sc["opacities"])
    bg = torch.tensor([r(0, 1), r(0, 1), r(0, 1)], device=device)
    xdt = torch.float16 if seed % 2 else None
    th = -(-H // 16)
    _, bands = band_plan(th, world)
    y0, y1 = min(bands[rank][0] * 16, H), min(bands[rank][1] * 16, H)
    arrays = lambda s_: (s_["means3d"], s_["scales"], s_["quats"], s_["opacities"], s_["features"])
    frames = []
    for k in range(10):
        a = 0.008 * k * (1 if seed % 3 else -1)
        c, s = math.cos(a), math.sin(a)
        ry = torch.tensor([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], device=device)
        cm = Camera(R=cam.R @ ry, T=cam.T + torch.tensor([0.0, 0.0, 0.015 * k], device=device), H=H, W=W, fx=cam.fx, fy=cam.fy,
                    cx=cam.cx, cy=cam.cy, near=cam.near, far=cam.far)
        frames.append((faint if 4 <= k < 7 else sc, cm))
    _hip_mod.config_depth_cut(0)
    refs = [ms.render_gaussians(*arrays(s_), cm, background_color=bg, backend="hip") for s_, cm in frames]
    _hip_mod.config_depth_cut(2)
    _fused._state.clear()
    _fused.FRAME_STATS = st = {}
    try:
        cur, k_cur = None, -1

        def check(b, k):
            want = refs[k][y0:y1] if xdt is None else refs[k][y0:y1].to(xdt)
            assert b.dtype == want.dtype and torch.equal(b[y0:y1], want), (seed, k, N, W, H, world, rank, dict(st))
        for k, (s_, cm) in enumerate(frames):
            nxt = render_gaussians_sharded(*arrays(s_), cm, background_color=bg, rehearse=(rank, world), async_op=True, exchange_dtype=xdt)
            if cur is not None:
                check(cur.wait(), k_cur)
            cur, k_cur = nxt, k
        check(cur.wait(), k_cur)
        torch.cuda.synchronize()
        assert st.get("regen_mismatch", 0) == 0, st
    finally:
        LAST_CUT_FUZZ_STATS.clear()
        LAST_CUT_FUZZ_STATS.update(_fused.FRAME_STATS or {})
        _fused.FRAME_STATS = None
        _fused._state.clear()


def test_claimed_rows_and_the_prefix_kernel_give_the_same_frames(device, tmp_path):
    """Round 6: the count kernel CLAIMS its stretch of every tile's segment with returning atomics (per-XCD-pair counters) and the
    prefix kernel is not launched (csrc/binning.hip, k_project_hist's tile_total; profiles/r06_claimed_rows.md).  Which
    workgroup gets which stretch changes where a pair sits in the UNSORTED buffer and nothing else: a child process with
    MOJOSPLAT_CLAIMED_ROWS=0 (the switch is read once) renders the same frames -- whole frames on all three binning grids,
    a band, a frame that overflows its buffer and is redone on the exact path, a depth-cut pair of frames -- bit for bit."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f'''
import sys, torch
sys.path.insert(0, {root!r})
import mojosplat_amd as ms
from mojosplat_amd import _fused, _hip
from mojosplat_amd.scenes import BACKGROUND_V1, randscene_v1
dev = torch.device("cuda", 0)
bg = torch.tensor(BACKGROUND_V1, device=dev)
out = {{}}
sc, cam = randscene_v1(150_000, 1024, 576, ell=-3.2, seed=5, device=dev)
g = (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])
for px in (16, 32, 64):
    for rep in range(3):   # (first frame: exact path; then sync-free frames on the learnt buffer)
        img = ms.render_gaussians(*g, cam, background_color=bg, bin_size=px)
    out[f"bin{{px}}"] = img.cpu()
_, m = _fused.render_fwd_hip(*g, cam, bg, 16, row_range=(5, 17))
out["band"] = _fused.render_fwd_hip(*g, cam, bg, 16, row_range=(5, 17))[0].cpu()
# a denser scene on the same lane: the speculated buffer overflows, the frame is redone exactly
sc2, cam2 = randscene_v1(150_000, 1024, 576, ell=-2.6, seed=6, device=dev)
g2 = (sc2["means3d"], sc2["scales"], sc2["quats"], sc2["opacities"], sc2["features"])
out["overflow"] = ms.render_gaussians(*g2, cam2, background_color=bg).cpu()
out["after"] = ms.render_gaussians(*g2, cam2, background_color=bg).cpu()
_hip.config_depth_cut(2, 0)
for rep in range(3):
    img = ms.render_gaussians(*g2, cam2, background_color=bg, bin_size=32)
out["cut"] = img.cpu()
out["cut_flag"] = int(_fused._dev_state(dev, 0)["host_np"][7]) & 64
torch.save(out, sys.argv[1])
'''
    outs = {}
    for claimed in ("1", "0"):
        path = str(tmp_path / f"frames_{claimed}.pt")
        env = dict(os.environ, MOJOSPLAT_CLAIMED_ROWS=claimed)
        r = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        outs[claimed] = torch.load(path)
    a, b = outs["1"], outs["0"]
    assert a["cut_flag"] and b["cut_flag"]          # (the last frames did take the depth cut)
    for k in a:
        if k != "cut_flag":
            assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["bin32"], a["overflow"])
