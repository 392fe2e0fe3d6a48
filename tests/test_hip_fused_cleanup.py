"""GPU: a bin of the fused sort + rasterise kernel (rasterize.hip, k_sort_rasterize) whose sorted front runs out with pixels
still alive fetches the rest of its list in the same workgroup -- no clean-up launch behind the frame (flag word bit 49,
kFrameCleanupInKernel) -- and the frame is, bit for bit, the frame that keeps the launch (fused-sort mode 2 | 4) and the
per-stage path's (fully sorted lists).

Images of 64x64 and 200x136 on 32-px bins; the fused path is forced with mode 2 as in test_hip_fused_sort.py, whose scene
builders are restated here (an anchor bin of 1100 faint specks keeps the frames off the light bet; the lane is put back on
the default front level after every frame, because a bin that walks on behind its front makes the lane ask for deeper
fronts, which keep the two launches).

The constants the cases are built around: a front is the nearest FRONT_K = 1024 entries rounded up to a whole depth bucket,
1536 .. FRONT_CAP = 2048 entries for these depth distributions (test_hip_fused_sort.py asserts the same window); every
further chunk holds at most CHUNK_CAP = 2048 entries (sort_device.hpp, kRedoCap).  So a bin of k entries whose front is f
walks on iff f < k, and needs at least two more chunks iff k - f > CHUNK_CAP.
"""
import numpy as np
import pytest
import torch

import mojosplat_amd as ms
import oracle
from helpers import check_image_strict, np_
from mojosplat_amd import _fused
from mojosplat_amd import _hip as _hip_mod
from mojosplat_amd.scenes import BACKGROUND_V1, randscene_v1
from mojosplat_amd.utils import Camera

pytestmark = pytest.mark.gpu

W, H, BIN = 200, 136, 32
TW, TH = 7, 5
FUSED_BIT, IN_KERNEL_BIT, DEPTH_CUT_BIT = 1 << 48, 1 << 49, 64
FRONT_LO, FRONT_CAP, CHUNK_CAP = 1536, 2048, 2048
BIN_XY = (3, 2)        # the controlled bin: x in [96, 128), y in [64, 96)
ANCHOR_XY = (1, 1)     # the anchor bin: x in [32, 64), y in [32, 64)
FX = 100.0
IN_KERNEL, KEPT = 2, 2 | 4   # fused-sort modes: forced; forced with the clean-up launch kept


@pytest.fixture(autouse=True)
def _default_settings_after_each_test():
    yield
    _hip_mod.config_fused_sort(1)
    _hip_mod.config_depth_cut(1, 6_000_000)
    _fused.FRAME_STATS = None
    _fused._state.clear()


def _camera(device):
    return Camera(R=torch.eye(3, device=device), T=torch.zeros(3, device=device), H=H, W=W, fx=FX, fy=FX, cx=W / 2, cy=H / 2)


def _specks(px, z, log_scale, opacity, gen):
    """Isotropic Gaussians whose centres project to the pixel positions px (n, 2) at depths z (n,)."""
    n = px.shape[0]
    means = torch.stack([(px[:, 0] - W / 2) * z / FX, (px[:, 1] - H / 2) * z / FX, z], 1)
    return dict(means3d=means, scales=torch.full((n, 3), float(log_scale)),
                quats=torch.nn.functional.normalize(torch.randn(n, 4, generator=gen), dim=1),
                opacities=opacity * (0.8 + 0.4 * torch.rand(n, generator=gen)), features=torch.rand(n, 3, generator=gen))


def _cat(parts):
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def _in_bin(px, bxy, margin):
    x0, y0 = bxy[0] * BIN, bxy[1] * BIN
    return (px[:, 0] > x0 - margin) & (px[:, 0] < x0 + BIN + margin) & (px[:, 1] > y0 - margin) & (px[:, 1] < y0 + BIN + margin)


def _scene(k, device, seed=0, bin_xy=BIN_XY, same_z=None, extra=None, n_bg=3000):
    """A sparse background that stays 6 px clear of the two special bins, the anchor bin's 1100 faint specks, and k faint
    specks (opacity ~0.005, sigma ~0.4 px: nothing saturates) in the controlled bin -- within 6 px of its centre, or, for a
    bin the image cuts at 8 px, of the centre of its visible strip.  same_z: all k at that depth.  extra(gen): more parts."""
    gen = torch.Generator().manual_seed(2000 + seed)
    px = torch.rand(n_bg, 2, generator=gen) * torch.tensor([float(W), float(H)])
    px = px[~(_in_bin(px, bin_xy, 6.0) | _in_bin(px, ANCHOR_XY, 6.0))]
    parts = [_specks(px, 4.0 + 4.0 * torch.rand(px.shape[0], generator=gen), -3.6, 0.6, gen)]
    centre = lambda bxy: torch.tensor([bxy[0] * BIN + BIN / 2.0, bxy[1] * BIN + BIN / 2.0])
    apx = centre(ANCHOR_XY) + 12.0 * (torch.rand(1100, 2, generator=gen) - 0.5)
    parts.append(_specks(apx, 4.0 + 4.0 * torch.rand(1100, generator=gen), -4.2, 0.01, gen))
    c, spread = centre(bin_xy), torch.tensor([12.0, 12.0])
    if (bin_xy[0] + 1) * BIN > W:   # the right edge: 8 visible columns
        c[0], spread[0] = bin_xy[0] * BIN + 4.0, 4.0
    if (bin_xy[1] + 1) * BIN > H:   # the bottom edge: 8 visible rows
        c[1], spread[1] = bin_xy[1] * BIN + 4.0, 4.0
    kpx = c + spread * (torch.rand(k, 2, generator=gen) - 0.5)
    z = torch.full((k,), float(same_z)) if same_z is not None else 4.0 + 4.0 * torch.rand(k, generator=gen)
    parts.append(_specks(kpx, z, -4.2, 0.005, gen))
    if extra is not None:
        parts += extra(gen)
    sc = {name: t.to(device) for name, t in _cat(parts).items()}
    return sc, _camera(device)


def _stack_scene(n, z_lo, z_hi, opacity, device, seed=0):
    """n big faint Gaussians piled up in front of the camera (test_hip_fused_sort.py's): every bin of a 64x64 image holds
    thousands of entries and none of them comes close to saturating a pixel."""
    g = torch.Generator().manual_seed(seed)
    means = torch.stack([torch.rand(n, generator=g) * 0.6 - 0.3, torch.rand(n, generator=g) * 0.6 - 0.3,
                         z_lo + (z_hi - z_lo) * torch.rand(n, generator=g)], 1)
    scales = torch.full((n, 3), -0.7) + 0.1 * torch.randn(n, 3, generator=g)
    quats = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=1)
    opac = opacity * (0.8 + 0.4 * torch.rand(n, generator=g))
    cols = torch.rand(n, 3, generator=g)
    cam = Camera(R=torch.eye(3, device=device), T=torch.zeros(3, device=device), H=64, W=64, fx=60.0, fy=60.0,
                 cx=32.0, cy=32.0)
    sc = dict(means3d=means, scales=scales, quats=quats, opacities=opac, features=cols)
    return {k: v.to(device) for k, v in sc.items()}, cam


def _g(sc):
    return (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])


def stagewise(sc, cam, bg, tile_size=BIN):
    m2, con, dep, rad = ms.project_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], cam, backend="hip")
    ids, ranges = ms.bin_gaussians_to_tiles(m2, rad, dep, cam.H, cam.W, tile_size, backend="hip")
    return ms.rasterize_gaussians(m2, con, sc["features"], sc["opacities"], bg, ranges, ids, cam, tile_size=tile_size,
                                  backend="hip")


def _flags(dev):
    return int(_fused._dev_state(dev, 0)["host_np"][7])


def _lane_back_to_default(dev):
    st = _fused._dev_state(dev, 0)
    st["full_sort"] = False
    st["front_level"] = 0


def _run(sc, cams, bg, mode):
    """One frame per camera on a fresh lane under fused-sort mode `mode` -> (images, flag words, frame statistics)."""
    dev = sc["means3d"].device
    _hip_mod.config_fused_sort(mode)
    _fused._state.clear()
    _fused.FRAME_STATS = stats = {}
    imgs, flags = [], []
    for cam in cams:
        imgs.append(ms.render_gaussians(*_g(sc), cam, background_color=bg, backend="hip", bin_size=BIN).clone())
        flags.append(_flags(dev))
        _lane_back_to_default(dev)
    _fused.FRAME_STATS = None
    return imgs, flags, stats


def _assert_paths(flags_in, flags_kept):
    """A lane's first frame sizes its buffers on the exact path; every frame after it is fused: the in-kernel frames carry
    bits 48 and 49, the frames that keep the launch bit 48 alone."""
    assert len(flags_in) >= 2 and len(flags_kept) >= 2
    for f in (flags_in[0], flags_kept[0]):
        assert f & 4 and not f & (FUSED_BIT | IN_KERNEL_BIT), hex(f)
    for f in flags_in[1:]:
        assert f & FUSED_BIT and f & IN_KERNEL_BIT, hex(f)
    for f in flags_kept[1:]:
        assert f & FUSED_BIT and not f & IN_KERNEL_BIT, hex(f)


def _three_way(sc, cam, bg, n_frames=3):
    """n frames in the kernel and n with the launch kept: all equal the per-stage path.  -> (image, statistics of the
    in-kernel run, the bins' ranges and front counts of its last frame)."""
    dev = sc["means3d"].device
    ref = stagewise(sc, cam, bg)
    kept, flags_kept, _ = _run(sc, [cam] * n_frames, bg, KEPT)
    inside, flags_in, stats = _run(sc, [cam] * n_frames, bg, IN_KERNEL)
    ranges, fronts = _fused.last_frame_lists(dev, sc["means3d"].shape[0], -(-cam.W // BIN), -(-cam.H // BIN))
    _assert_paths(flags_in, flags_kept)
    for i in range(n_frames):
        assert torch.equal(inside[i], kept[i]), i
        assert torch.equal(inside[i], ref), (i, float((inside[i] - ref).abs().max()))
    assert stats.get("cleanup_in_kernel", 0) == n_frames - 1 and stats.get("fused_sort", 0) == n_frames - 1, stats
    return inside[-1], stats, ranges, fronts


def test_stranded_bins_finish_in_the_kernel(device):
    """1. 4000 faint Gaussians over 64x64: every bin's front leaves its pixels alive and every bin walks on to the end of its
    list; the bins are reported as redone one frame later, as behind the clean-up launch."""
    sc, cam = _stack_scene(4000, 4.0, 6.0, 0.005, device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    _, stats, ranges, fronts = _three_way(sc, cam, bg, n_frames=4)
    n = ranges[..., 1] - ranges[..., 0]
    assert int(n.min()) > FRONT_CAP and bool((fronts < n).all()), (n, fronts)   # all four bins are short of their lists
    assert stats.get("redo_tiles", 0) >= 8, stats   # (four bins a fused frame, reported one frame late: by frames 2 and 3)


@pytest.mark.parametrize("k", [1537, 2049, 3000, 4097, 6000])
def test_controlled_bin_on_both_sides_of_the_front_and_of_the_chunk_edges(device, k):
    """2. One bin of k faint specks."""
    sc, cam = _scene(k, device, seed=k)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    img, stats, ranges, fronts = _three_way(sc, cam, bg)
    n = ranges[..., 1] - ranges[..., 0]
    n_bin, n_anchor = int(n[BIN_XY[1], BIN_XY[0]]), int(n[ANCHOR_XY[1], ANCHOR_XY[0]])
    assert n_bin == k and 1024 < n_anchor <= 1100 and int(n.max()) == max(k, n_anchor), (n_bin, n_anchor)
    f = int(fronts[BIN_XY[1], BIN_XY[0]])   # (the first front's: a bin that walks on leaves it as it was)
    assert FRONT_LO <= f <= FRONT_CAP and f <= k, (f, k)
    if k >= 2049:
        assert f < k                       # walks on ...
    if k in (4097, 6000):
        assert k - f > CHUNK_CAP           # ... through two more chunks at least
    if k in (2049, 3000):
        assert k - f <= CHUNK_CAP          # ... through one (the rest fits one chunk's room)
    if f < k:
        assert stats.get("redo_tiles", 0) >= 1, stats   # the bin's pixels are alive behind its front: frame 2 reports frame 1's


def test_in_kernel_frame_against_the_oracle(device):
    """8. The controlled bin of 3000 faint specks, finished in the kernel, against the CPU oracle under the suite's
    end-to-end bar -- the one reference here that shares no code with the HIP paths."""
    sc, cam = _scene(3000, device, seed=3000)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    imgs, flags, _ = _run(sc, [cam] * 2, bg, IN_KERNEL)
    assert flags[1] & FUSED_BIT and flags[1] & IN_KERNEL_BIT, hex(flags[1])
    cpu = {name: np_(v) for name, v in sc.items()}
    ref, aux = oracle.render_fwd(cpu["means3d"], cpu["scales"], cpu["quats"], cpu["opacities"], cpu["features"],
                                 np_(cam.view_matrix), cam.fx, cam.fy, cam.cx, cam.cy, W, H,
                                 background=np.array(BACKGROUND_V1, np.float32), margin=True)
    check_image_strict(imgs[1], ref, aux["margin"], tag="short front finished in the kernel, 200x136 on 32-px bins", eps=2e-5)


def test_bit_equal_depths_are_ordered_by_id(device):
    """3. 3000 faint specks at one z under the identity camera: equal depth bits, so the front selection finds one crowded
    bucket and the next chunk's selection has to narrow into the id half of the keys."""
    k = 3000
    sc, cam = _scene(k, device, seed=33, same_z=5.0)
    _, _, dep, _ = ms.project_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], cam, backend="hip")
    assert int(torch.unique(dep[-k:].view(torch.int32)).numel()) == 1
    bg = torch.tensor(BACKGROUND_V1, device=device)
    _, stats, ranges, fronts = _three_way(sc, cam, bg)
    assert int((ranges[..., 1] - ranges[..., 0])[BIN_XY[1], BIN_XY[0]]) == k
    assert int(fronts[BIN_XY[1], BIN_XY[0]]) < k and stats.get("redo_tiles", 0) >= 1, (fronts, stats)


def test_finished_quad_keeps_its_pixels_while_the_others_walk_on(device):
    """4. Five near layers of opaque specks over one 8x8 quad of the controlled bin finish it inside the first front; the
    bin's other quads see only the 6000 faint specks and stay alive through two more chunks."""
    qx, qy = BIN_XY[0] * BIN + 8, BIN_XY[1] * BIN + 8   # the quad [104, 112) x [72, 80): inside the faint specks' patch

    def cluster(gen):
        ys, xs = torch.meshgrid(torch.arange(8.0), torch.arange(8.0), indexing="ij")
        px = torch.stack([qx + 0.5 + xs.reshape(-1), qy + 0.5 + ys.reshape(-1)], 1).repeat(5, 1)
        z = 2.0 + 0.2 * torch.arange(5.0).repeat_interleave(64) + 0.01 * torch.rand(320, generator=gen)
        p = _specks(px, z, -3.6, 0.95, gen)
        p["opacities"] = torch.full((320,), 0.95)
        return [p]

    k = 6000
    sc, cam = _scene(k, device, seed=44, extra=cluster)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    # the class that was meant: the quad's pixels do not see the background (finished), its bin's other pixels do
    a, b = stagewise(sc, cam, bg), stagewise(sc, cam, 1.0 - bg)
    d = (a - b).abs().amax(-1)
    # (a pixel stops before the entry that would take T (1 - alpha) to 1e-4 or below, so a finished pixel under entries of
    # alpha <= 0.95 keeps T <= 1e-4 / 0.05 = 2e-3 -- each pixel centre carries its own speck in every layer: the fourth stops it)
    assert float(d[qy:qy + 8, qx:qx + 8].max()) <= 2e-3
    y0, x0 = BIN_XY[1] * BIN, BIN_XY[0] * BIN
    alive = d[y0:y0 + BIN, x0:x0 + BIN].reshape(4, 8, 4, 8).amax(dim=(1, 3))   # per quad: its most transparent pixel
    alive[(qy - y0) // 8, (qx - x0) // 8] = 1.0
    assert float(alive.min()) > 0.05   # every other quad of the bin keeps a live pixel (the cluster's tails finish a few neighbours)
    _, stats, ranges, fronts = _three_way(sc, cam, bg)
    n_bin, f = int((ranges[..., 1] - ranges[..., 0])[BIN_XY[1], BIN_XY[0]]), int(fronts[BIN_XY[1], BIN_XY[0]])
    assert n_bin == k + 320 and FRONT_LO <= f <= FRONT_CAP and n_bin - f > CHUNK_CAP, (n_bin, f)
    assert stats.get("redo_tiles", 0) >= 1, stats


@pytest.mark.parametrize("bin_xy", [(TW - 1, 2), (3, TH - 1)], ids=["right_edge", "bottom_edge"])
def test_bins_the_image_cuts(device, bin_xy):
    """5. The controlled bin at the right and at the bottom edge of 200x136: 8 of its 32 columns (rows) are inside the image,
    two of its four blocks lie wholly outside -- their waves walk nothing and still take every barrier."""
    k = 3000
    sc, cam = _scene(k, device, seed=50 + bin_xy[0], bin_xy=bin_xy)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    _, stats, ranges, fronts = _three_way(sc, cam, bg)
    n_bin, f = int((ranges[..., 1] - ranges[..., 0])[bin_xy[1], bin_xy[0]]), int(fronts[bin_xy[1], bin_xy[0]])
    assert n_bin == k and FRONT_LO <= f <= FRONT_CAP, (n_bin, f)
    assert stats.get("redo_tiles", 0) >= 1, stats


def test_eight_poses_on_one_lane(device):
    """6. A camera that turns a little every frame over the stack of faint Gaussians: bins walk on in every frame, and every
    frame equals the frame that keeps the launch."""
    sc, cam0 = _stack_scene(4000, 4.0, 6.0, 0.005, device, seed=6)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    cams = []
    for i in range(8):
        a = 0.01 * i
        rot = torch.tensor([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]], dtype=torch.float32, device=device)
        cams.append(Camera(R=cam0.R @ rot, T=cam0.T, H=cam0.H, W=cam0.W, fx=cam0.fx, fy=cam0.fy, cx=cam0.cx, cy=cam0.cy))
    kept, flags_kept, _ = _run(sc, cams, bg, KEPT)
    inside, flags_in, stats = _run(sc, cams, bg, IN_KERNEL)
    _assert_paths(flags_in, flags_kept)
    for i in range(8):
        assert torch.equal(inside[i], kept[i]), i
    assert torch.equal(inside[7], stagewise(sc, cams[7], bg))
    assert stats.get("cleanup_in_kernel", 0) == 7 and stats.get("redo_tiles", 0) >= 6, stats


def test_depth_cut_frames_keep_the_launches(device):
    """7. With the depth cut forced, the fused frames that drop pairs behind their bins' cut-offs keep the clean-up launches
    (only those bring the pairs back): bit 49 clear on them, the image the per-stage path's."""
    sc, cam = randscene_v1(40_000, W, H, ell=-2.6, seed=11, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    _hip_mod.config_depth_cut(2, 0)
    ref = stagewise(sc, cam, bg)
    imgs, flags, _ = _run(sc, [cam] * 5, bg, IN_KERNEL)
    assert all(f & FUSED_BIT for f in flags[1:]), [hex(f) for f in flags]
    cut = [f for f in flags if f & DEPTH_CUT_BIT]
    assert cut and all(f & FUSED_BIT and not f & IN_KERNEL_BIT for f in cut), [hex(f) for f in flags]
    assert all(bool(f & IN_KERNEL_BIT) == (not f & DEPTH_CUT_BIT) for f in flags if f & FUSED_BIT), [hex(f) for f in flags]
    for i, img in enumerate(imgs):
        assert torch.equal(img, ref), i
