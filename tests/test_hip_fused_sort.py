"""GPU: the frame whose bins are sorted by the workgroups that rasterise them (rasterize.hip, k_sort_rasterize: one
launch instead of the merged sort launch followed by the rasteriser) is the frame of the two launches, bit for bit.

The image is 200x136 on 32-px bins: 7x5 bins with ragged right and bottom edges of 8 px.  By its own rule the rasteriser
runs two waves a block -- and the library fuses -- only from a whole 1080p frame on (rasterize.hip, choose_parts), so the
tests ask for the fused path on every frame that can structurally take it (config_fused_sort(2)) and assert from the
frame's flag word (bit 48, kFrameFusedSort) that it was really taken; the default rule at full size is exercised by
test_hip_configs.py / test_hip_cameras.py and bench.py.

A frame with no bin beyond 1024 entries is a light-bet frame from its second frame on (only the small sort launch, no
fronts: pipeline.hip, bet_light) and keeps its launches; the scenes here therefore carry one ANCHOR bin of 1100 specks that
is selected whole and saturates nothing, so that the controlled bin's own class -- empty, light, short, heavy -- is what
varies.  A bin whose sorted front is shorter than its list strands its unsaturated pixels: the lane then asks for deeper
fronts (which keep the two launches), so the loops put the lane back on the default level after every frame, as
test_hip_fused.py::test_two_launch_clean_up_on_coarse_bins does.
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
FUSED_BIT = 1 << 48
BIN_XY = (3, 2)        # the controlled bin: x in [96, 128), y in [64, 96)
ANCHOR_XY = (1, 1)     # the anchor bin: x in [32, 64), y in [32, 64)
FX = 100.0


@pytest.fixture(autouse=True)
def _default_settings_after_each_test():
    """Tests switch the library's fused-sort mode (and one its depth-cut mode) in-process; every test leaves the defaults
    and no lane state behind."""
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


def _scene(k, device, seed=0, opacity=0.5, n_bg=3000):
    """A sparse background of small Gaussians that stays 6 px clear of the two special bins, the anchor bin's 1100 faint
    specks, and k tiny Gaussians (sigma ~ 0.4 px: a footprint of a few pixels) within 6 px of the controlled bin's centre."""
    gen = torch.Generator().manual_seed(1000 + seed)
    px = torch.rand(n_bg, 2, generator=gen) * torch.tensor([float(W), float(H)])
    px = px[~(_in_bin(px, BIN_XY, 6.0) | _in_bin(px, ANCHOR_XY, 6.0))]
    parts = [_specks(px, 4.0 + 4.0 * torch.rand(px.shape[0], generator=gen), -3.6, 0.6, gen)]
    centre = lambda bxy: torch.tensor([bxy[0] * BIN + BIN / 2.0, bxy[1] * BIN + BIN / 2.0])
    apx = centre(ANCHOR_XY) + 12.0 * (torch.rand(1100, 2, generator=gen) - 0.5)
    parts.append(_specks(apx, 4.0 + 4.0 * torch.rand(1100, generator=gen), -4.2, 0.01, gen))
    if k:
        kpx = centre(BIN_XY) + 12.0 * (torch.rand(k, 2, generator=gen) - 0.5)
        parts.append(_specks(kpx, 4.0 + 4.0 * torch.rand(k, generator=gen), -4.2, opacity, gen))
    sc = {name: t.to(device) for name, t in _cat(parts).items()}
    return sc, _camera(device)


def _g(sc):
    return (sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"])


def stagewise(sc, cam, bg, tile_size=BIN):
    m2, con, dep, rad = ms.project_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], cam, backend="hip")
    ids, ranges = ms.bin_gaussians_to_tiles(m2, rad, dep, cam.H, cam.W, tile_size, backend="hip")
    if ids.numel() == 0:
        return torch.zeros(cam.H, cam.W, sc["features"].shape[1], device=m2.device)
    return ms.rasterize_gaussians(m2, con, sc["features"], sc["opacities"], bg, ranges, ids, cam, tile_size=tile_size,
                                  backend="hip")


def _flags(dev):
    """The flag word of the last frame on the lane of `dev` (a tensor's device: the key the lanes are kept under)."""
    return int(_fused._dev_state(dev, 0)["host_np"][7])


def _lane_back_to_default(dev):
    st = _fused._dev_state(dev, 0)
    st["full_sort"] = False
    st["front_level"] = 0


def _frames(sc, cam, bg, mode, n_frames=3, **kw):
    """n frames on a fresh lane under fused-sort mode `mode` -> (last image, its flag word, the bins' ranges, front counts)."""
    dev = sc["means3d"].device
    _hip_mod.config_fused_sort(mode)
    _fused._state.clear()
    img = None
    for _ in range(n_frames):
        img = ms.render_gaussians(*_g(sc), cam, background_color=bg, backend="hip", **kw)
        _lane_back_to_default(dev)
    flags = _flags(dev)
    ranges, fronts = _fused.last_frame_lists(dev, sc["means3d"].shape[0], TW, TH)
    return img, flags, ranges, fronts


_ORACLE_CHECKED = []


# (list length of the controlled bin, its class, whether its sorted front is shorter than its list)
@pytest.mark.parametrize("k,cls", [(0, "empty"), (1, "light"), (255, "light"), (256, "short"), (1024, "short"),
                                   (1025, "whole"), (1536, "whole"), (1537, "front"), (3000, "front")])
def test_fused_frame_equals_the_two_launches_for_every_class_of_bin(device, k, cls):
    sc, cam = _scene(k, device, seed=k)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    on, flags_on, ranges_on, fronts_on = _frames(sc, cam, bg, 2, bin_size=BIN)
    off, flags_off, ranges_off, fronts_off = _frames(sc, cam, bg, 0, bin_size=BIN)
    # the class that was meant: the controlled bin holds exactly the k specks, the anchor bin is heavy and selected whole
    n = ranges_on[..., 1] - ranges_on[..., 0]
    n_bin, n_anchor = int(n[BIN_XY[1], BIN_XY[0]]), int(n[ANCHOR_XY[1], ANCHOR_XY[0]])
    assert n_bin == k and 1024 < n_anchor <= 1100, (n_bin, n_anchor)
    assert int(n.max()) == max(k, n_anchor)
    f_bin = int(fronts_on[BIN_XY[1], BIN_XY[0]])
    if cls == "whole":
        assert f_bin == k
    elif cls == "front":
        assert 1536 <= f_bin <= 2048 and (f_bin < k or k == 1537), (f_bin, k)   # (1537: the bucket that completes the front may hold the last entry)
        if k == 3000:
            assert f_bin < k
    # 1. the path was really taken (and not with the switch off)
    assert flags_on & FUSED_BIT and not flags_off & FUSED_BIT, (hex(flags_on), hex(flags_off))
    # 2. / 3. the same image as the two launches and as the per-stage path
    assert torch.equal(on, off)
    assert torch.equal(on, stagewise(sc, cam, bg))
    # 4. the same lists: ranges everywhere, front counts where a bin has one (lists beyond 1024 entries)
    assert torch.equal(ranges_on, ranges_off)
    heavy = n > 1024
    assert torch.equal(fronts_on[heavy], fronts_off[heavy])
    # 5. once for the whole file: the oracle, under the suite's end-to-end bar
    if not _ORACLE_CHECKED and k == 1025:
        cpu = {name: np_(v) for name, v in sc.items()}
        ref, aux = oracle.render_fwd(cpu["means3d"], cpu["scales"], cpu["quats"], cpu["opacities"], cpu["features"],
                                     np_(cam.view_matrix), cam.fx, cam.fy, cam.cx, cam.cy, W, H,
                                     background=np.array(BACKGROUND_V1, np.float32), margin=True)
        check_image_strict(on, ref, aux["margin"], tag="fused sort + rasterise, 200x136 on 32-px bins", eps=2e-5)
        _ORACLE_CHECKED.append(k)


def _stack_scene(n, z_lo, z_hi, opacity, device, seed=0):
    """n big faint Gaussians piled up in front of the camera (as test_hip_fused.py's): every bin of a 64x64 image holds
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


def test_stranded_bins_go_through_the_clean_up_launch(device):
    """4000 faint Gaussians over a 64x64 image: every 32-px bin's 1536-entry front leaves its pixels alive, the fused
    kernel's waves put the bin on the redo list as the rasteriser's do, and the clean-up launch redoes it."""
    sc, cam = _stack_scene(4000, 4.0, 6.0, 0.005, device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    ref = stagewise(sc, cam, bg)
    _hip_mod.config_fused_sort(2)
    _fused._state.clear()
    _fused.FRAME_STATS = stats = {}
    for _ in range(4):
        img = ms.render_gaussians(*_g(sc), cam, background_color=bg, backend="hip", bin_size=BIN)
        assert torch.equal(img, ref)
        _lane_back_to_default(sc["means3d"].device)
    assert _flags(sc["means3d"].device) & FUSED_BIT
    assert stats.get("fused_sort", 0) >= 2 and stats.get("redo_tiles", 0) > 0, stats   # (redone bins are reported one frame late)


def test_scene_swap_overflow_and_exact_redo_then_fused_again(device):
    """A small scene, then a much larger one on the same lane: the buffer sized by the first overflows under the fused
    kernel (its workgroups leave the bins beyond the capacity unsorted and render nothing of them), the frame is redone
    on the exact path, and the frames after it are fused again."""
    bg = torch.tensor(BACKGROUND_V1, device=device)
    small, cam = _scene(10, device, seed=1, n_bg=500)
    big, _ = _scene(3000, device, seed=2, n_bg=30000)
    _hip_mod.config_fused_sort(2)
    _fused._state.clear()
    _fused.FRAME_STATS = stats = {}
    ref_small, ref_big = stagewise(small, cam, bg), stagewise(big, cam, bg)
    for _ in range(2):
        assert torch.equal(ms.render_gaussians(*_g(small), cam, background_color=bg, backend="hip", bin_size=BIN), ref_small)
    assert _flags(small["means3d"].device) & FUSED_BIT
    for i in range(3):
        assert torch.equal(ms.render_gaussians(*_g(big), cam, background_color=bg, backend="hip", bin_size=BIN), ref_big), i
        _lane_back_to_default(big["means3d"].device)
    assert stats.get("overflow", 0) >= 1 and stats.get("redone_exact", 0) >= 1, stats
    assert _flags(big["means3d"].device) & FUSED_BIT


def test_orbit_of_eight_poses_on_one_lane(device):
    sc, cam0 = randscene_v1(40_000, W, H, ell=-2.6, seed=11, device=device)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    _hip_mod.config_fused_sort(2)
    _fused._state.clear()
    _fused.FRAME_STATS = stats = {}
    centre = sc["means3d"].mean(0)
    for i in range(8):
        a = 0.05 * i
        rot = torch.tensor([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]], dtype=torch.float32, device=device)
        R = cam0.R @ rot
        T = cam0.T + cam0.R @ (centre - rot @ centre)
        cam = Camera(R=R, T=T, H=H, W=W, fx=cam0.fx, fy=cam0.fy, cx=cam0.cx, cy=cam0.cy)
        img = ms.render_gaussians(*_g(sc), cam, background_color=bg, backend="hip", bin_size=BIN)
        assert torch.equal(img, stagewise(sc, cam, bg)), i
        _lane_back_to_default(sc["means3d"].device)
    assert stats.get("fused_sort", 0) >= 4, stats


@pytest.mark.parametrize("what", ["bin64", "bin16_split", "band", "trainable"])
def test_frames_that_keep_the_two_launches(device, what):
    """64-px bins, a split frame (16-px tiles cut from 32-px bins), a band of bin rows and a differentiable frame: none
    carries the bit, each is the same frame with the switch on and off."""
    sc, cam = _scene(1537, device, seed=5)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    dev = sc["means3d"].device

    def frame():
        if what == "bin64":
            return ms.render_gaussians(*_g(sc), cam, background_color=bg, backend="hip", bin_size=64)
        if what == "bin16_split":
            return ms.render_gaussians(*_g(sc), cam, background_color=bg, backend="hip", bin_size=16)
        if what == "band":
            out = torch.full((TH * BIN, W, 3), -1.0, device=dev)
            _fused.render_fwd_hip(*_g(sc), cam, bg, BIN, row_range=(1, 4), out=out)
            return out
        from mojosplat_amd.autograd import render_gaussians_trainable
        leaves = [t.clone().requires_grad_(True) for t in _g(sc)]
        return render_gaussians_trainable(*leaves, cam, background_color=bg, tile_size=BIN).detach()

    got = {}
    for mode in (2, 0):
        _hip_mod.config_fused_sort(mode)
        _fused._state.clear()
        for _ in range(3):
            img = frame()
            assert not _flags(dev) & FUSED_BIT, (what, mode, hex(_flags(dev)))
            _lane_back_to_default(dev)
        got[mode] = img.clone()
    assert torch.equal(got[2], got[0])
    if what in ("bin64", "bin16_split"):
        assert torch.equal(got[2], stagewise(sc, cam, bg, 16))
