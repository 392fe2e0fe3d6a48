"""GPU: the sort phase of the fused rasteriser (rasterize.hip, k_sort_rasterize) after its chain of memory round trips was
shortened -- one record per order position instead of order[] -> tile_ranges[], the frame's depth range asked for at the
kernel's first instruction and reduced behind the barrier that publishes the zeroed counters, the list's first
kLoads * THREADS keys kept in registers from the histogram to the selection (sort_device.hpp, front_select_lds), fewer
barriers -- is exact: at every list length where one of those pieces can go wrong, the fused frame is the frame of the
two launches and of the per-stage path (fully sorted lists, an independent sort), bit for bit, and leaves the same ranges
and front counts.

Shape and scenes as in test_hip_fused_sort.py: 200x136 on 32-px bins (7x5 bins, ragged right and bottom edges), one ANCHOR
bin of 1100 specks so that no frame is a light-bet frame, and a CONTROLLED bin whose list is what varies -- here not only
in length but in its depths (a crowd at one bit-equal depth, a list of one depth).  The lengths come from the constants of
the source the library was built from.
"""
import re
from pathlib import Path

import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import _fused
from mojosplat_amd import _hip as _hip_mod
from mojosplat_amd.scenes import BACKGROUND_V1
from mojosplat_amd.utils import Camera

pytestmark = pytest.mark.gpu

W, H, BIN = 200, 136, 32
TW, TH = 7, 5
FUSED_BIT = 1 << 48
BIN_XY = (3, 2)        # the controlled bin: x in [96, 128), y in [64, 96)
ANCHOR_XY = (1, 1)     # the anchor bin: x in [32, 64), y in [32, 64)
N_ANCHOR = 1100
FX = 100.0

_CSRC = Path(ms.__file__).parent / "csrc"


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


_SORT, _RAST = (_CSRC / "sort_device.hpp").read_text(), (_CSRC / "rasterize.hip").read_text()
FRONT_K = _const(_SORT, r"constexpr int kFrontK = (\d+);")                    # lists up to here are sorted whole
BUCKET_FALLBACK = _const(_SORT, r"constexpr int kBucketFallback = (\d+);")    # a bucket more crowded than this: bitonic
FUSED_THREADS = _const(_RAST, r"constexpr int kFusedThreads = (\d+),")
FUSED_CAP = _const(_RAST, r"kFusedCap = (\d+);")                              # ids of LDS room: the front's cap
LOADS = _const(_RAST, r"front_select_lds<kFusedThreads, (\d+)>")              # keys a thread keeps in registers
REGS = LOADS * FUSED_THREADS
# the lane's front depth on plain 32-px bins at the default front level (binning.hip, front_params: blocks_per_tile == 4)
LANE_FRONT_K = _const((_CSRC / "binning.hip").read_text(), r"blocks_per_tile == 4 \? (\d+) :")


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
    """Isotropic Gaussians whose centres project to the pixel positions px (n, 2) at depths z (n,): the camera looks down
    +z from the origin, so a Gaussian's depth IS z, bit for bit."""
    n = px.shape[0]
    means = torch.stack([(px[:, 0] - W / 2) * z / FX, (px[:, 1] - H / 2) * z / FX, z], 1)
    return dict(means3d=means, scales=torch.full((n, 3), float(log_scale)),
                quats=torch.nn.functional.normalize(torch.randn(n, 4, generator=gen), dim=1),
                opacities=opacity * (0.8 + 0.4 * torch.rand(n, generator=gen)), features=torch.rand(n, 3, generator=gen))


def _in_bin(px, bxy, margin):
    x0, y0 = bxy[0] * BIN, bxy[1] * BIN
    return (px[:, 0] > x0 - margin) & (px[:, 0] < x0 + BIN + margin) & (px[:, 1] > y0 - margin) & (px[:, 1] < y0 + BIN + margin)


def _centre(bxy):
    return torch.tensor([bxy[0] * BIN + BIN / 2.0, bxy[1] * BIN + BIN / 2.0])


def _scene(depths, device, seed=0, opacity=0.5, n_bg=3000):
    """A sparse background that stays 6 px clear of the two special bins, the anchor bin's faint specks, and one tiny
    Gaussian (sigma ~ 0.4 px) per entry of `depths` (a length: that many random depths in [4, 8)) within 6 px of the
    controlled bin's centre."""
    gen = torch.Generator().manual_seed(2000 + seed)
    parts = []
    if n_bg:
        px = torch.rand(n_bg, 2, generator=gen) * torch.tensor([float(W), float(H)])
        px = px[~(_in_bin(px, BIN_XY, 6.0) | _in_bin(px, ANCHOR_XY, 6.0))]
        parts.append(_specks(px, 4.0 + 4.0 * torch.rand(px.shape[0], generator=gen), -3.6, 0.6, gen))
    apx = _centre(ANCHOR_XY) + 12.0 * (torch.rand(N_ANCHOR, 2, generator=gen) - 0.5)
    parts.append(_specks(apx, 4.0 + 4.0 * torch.rand(N_ANCHOR, generator=gen), -4.2, 0.01, gen))
    if isinstance(depths, int):
        depths = 4.0 + 4.0 * torch.rand(depths, generator=gen)
    k = depths.shape[0]
    if k:
        kpx = _centre(BIN_XY) + 12.0 * (torch.rand(k, 2, generator=gen) - 0.5)
        parts.append(_specks(kpx, depths.float(), -4.2, opacity, gen))
    sc = {name: torch.cat([p[name] for p in parts]).to(device) for name in parts[0]}
    return sc, _camera(device)


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
    """A bin whose front is shorter than its list makes the lane ask for deeper fronts, which keep the two launches."""
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


def _near_then_crowd(n_near, n_crowd, z_crowd=6.0, seed=7):
    """n_near distinct depths in [4, 5.5), then n_crowd entries at ONE bit-equal depth behind them."""
    gen = torch.Generator().manual_seed(seed)
    return torch.cat([4.0 + 1.5 * torch.rand(n_near, generator=gen), torch.full((n_crowd,), float(z_crowd))])


# name -> the controlled bin's depths (a length: random depths).  The smallest lengths at which each piece can go wrong:
CASES = {
    "empty": 0,
    "one": 1,
    "whole_sort_last": FRONT_K,                    # sort_segment_lds | front_select_lds
    "selection_first": FRONT_K + 1,
    "front_k": LANE_FRONT_K,                       # selected whole | a front shorter than the list may begin
    "front_k_plus_1": LANE_FRONT_K + 1,
    "regs_minus_1": REGS - 1,                      # every key in registers ...
    "regs": REGS,
    "regs_plus_1": REGS + 1,                       # ... | a remainder of one key read again
    "two_rounds_plus_1": 2 * REGS + 1,             # a second full round of the remainder's loop, and one key more
    # longer than the room, and the bucket that completes the front overflows it: the front steps one bucket back
    "step_back": _near_then_crowd(LANE_FRONT_K - 500, FUSED_CAP - LANE_FRONT_K + 600),
    # a short list with more than kBucketFallback entries at one depth: the bitonic network
    "bitonic": _near_then_crowd(100, BUCKET_FALLBACK + 88),
    # one depth for the whole list (span 0): a short list below the bitonic threshold, and a heavy one
    "span0_short": torch.full((300,), 5.0),
    "span0_heavy": torch.full((FRONT_K + 76,), 5.0),
}


def test_the_cases_sit_on_the_code_s_boundaries():
    assert FUSED_THREADS == 512 and FRONT_K < LANE_FRONT_K < REGS <= FUSED_CAP
    # (step_back: the crowd's bucket begins before the front is complete and ends beyond the room)
    assert LANE_FRONT_K - 500 < LANE_FRONT_K and CASES["step_back"].shape[0] > FUSED_CAP
    assert CASES["bitonic"].shape[0] <= FRONT_K and CASES["span0_short"].shape[0] <= BUCKET_FALLBACK


@pytest.mark.parametrize("name", list(CASES))
def test_fused_frame_is_exact_at_every_boundary_of_the_sort_chain(device, name):
    depths = CASES[name]
    k = depths if isinstance(depths, int) else depths.shape[0]
    sc, cam = _scene(depths, device, seed=k)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    on, flags_on, ranges_on, fronts_on = _frames(sc, cam, bg, 2, bin_size=BIN)
    off, flags_off, ranges_off, fronts_off = _frames(sc, cam, bg, 0, bin_size=BIN)
    n = ranges_on[..., 1] - ranges_on[..., 0]
    assert int(n[BIN_XY[1], BIN_XY[0]]) == k and FRONT_K < int(n[ANCHOR_XY[1], ANCHOR_XY[0]]) <= N_ANCHOR
    assert flags_on & FUSED_BIT and not flags_off & FUSED_BIT, (hex(flags_on), hex(flags_off))
    assert torch.equal(on, off)
    assert torch.equal(on, stagewise(sc, cam, bg))
    assert torch.equal(ranges_on, ranges_off)
    heavy = n > FRONT_K
    assert torch.equal(fronts_on[heavy], fronts_off[heavy])
    f_bin = int(fronts_on[BIN_XY[1], BIN_XY[0]])
    if FRONT_K < k <= LANE_FRONT_K or name == "span0_heavy":
        assert f_bin == k                                  # selected whole
    elif name == "step_back":
        assert f_bin == LANE_FRONT_K - 500                 # the crowd's bucket did not fit: the front ends before it
    elif k > LANE_FRONT_K:
        assert LANE_FRONT_K <= f_bin <= FUSED_CAP, f_bin


def _padded(sc, n_total):
    """`sc` with Gaussians behind the camera (culled by the projection) appended up to n_total: the lane keeps one shape."""
    pad = n_total - sc["means3d"].shape[0]
    if pad == 0:
        return sc
    dev = sc["means3d"].device
    extra = dict(means3d=torch.tensor([0.0, 0.0, -5.0], device=dev).repeat(pad, 1), scales=torch.full((pad, 3), -4.2, device=dev),
                 quats=torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev).repeat(pad, 1), opacities=torch.full((pad,), 0.5, device=dev),
                 features=torch.zeros(pad, 3, device=dev))
    return {name: torch.cat([sc[name], extra[name]]) for name in sc}


def test_three_frames_on_one_lane_with_a_changing_bin(device):
    """Behind two frames that size the lane's buffers, three consecutive frames whose controlled bin changes its length
    (one key, a front shorter than its list, empty), each from scene tensors of its own: nothing of a frame's per-position
    records may outlive it.  Every frame is compared with the per-stage path, the lists of each with the two launches'."""
    bg = torch.tensor(BACKGROUND_V1, device=device)
    ks = (2 * REGS + 1, 2 * REGS + 1, 1, LANE_FRONT_K + 1, 0)
    scenes = [_scene(k, device, seed=10 + i) for i, k in enumerate(ks)]
    n_total = max(sc["means3d"].shape[0] for sc, _ in scenes)
    scenes = [(_padded(sc, n_total), cam) for sc, cam in scenes]
    refs = [stagewise(sc, cam, bg) for sc, cam in scenes]
    lists = {2: [], 0: []}
    for mode in (2, 0):
        _hip_mod.config_fused_sort(mode)
        _fused._state.clear()
        for i, ((sc, cam), ref) in enumerate(zip(scenes, refs)):
            dev = sc["means3d"].device
            img = ms.render_gaussians(*_g(sc), cam, background_color=bg, backend="hip", bin_size=BIN)
            _lane_back_to_default(dev)
            assert torch.equal(img, ref), (mode, i)
            if i >= 2:
                assert bool(_flags(dev) & FUSED_BIT) == (mode == 2), (mode, i, hex(_flags(dev)))
                lists[mode].append(_fused.last_frame_lists(dev, n_total, TW, TH))
    for k, (r_on, f_on), (r_off, f_off) in zip(ks[2:], lists[2], lists[0]):
        n = r_on[..., 1] - r_on[..., 0]
        assert int(n[BIN_XY[1], BIN_XY[0]]) == k
        assert torch.equal(r_on, r_off) and torch.equal(f_on[n > FRONT_K], f_off[n > FRONT_K])


def test_empty_bins_behind_the_last_non_empty_one(device):
    """No background: two bins hold everything and 33 empty ones fill the order behind them."""
    sc, cam = _scene(LANE_FRONT_K + 1, device, seed=3, n_bg=0)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    on, flags_on, ranges_on, fronts_on = _frames(sc, cam, bg, 2, bin_size=BIN)
    off, _, ranges_off, fronts_off = _frames(sc, cam, bg, 0, bin_size=BIN)
    n = ranges_on[..., 1] - ranges_on[..., 0]
    assert int((n > 0).sum()) == 2 and flags_on & FUSED_BIT
    assert torch.equal(on, off) and torch.equal(on, stagewise(sc, cam, bg))
    assert torch.equal(ranges_on, ranges_off) and torch.equal(fronts_on[n > FRONT_K], fronts_off[n > FRONT_K])


@pytest.mark.parametrize("bin_size", [64, 16])
def test_the_front_kernel_s_use_of_the_selection_outside_the_fused_kernel(device, bin_size):
    """k_tile_front calls the same routine: the merged launch on 64-px bins (kLoads = 4: a remainder read again) and the
    split frame's front launch (16-px tiles cut from 32-px bins, kLoads = 8: every key in registers).  Two launches."""
    sc, cam = _scene(REGS + 952, device, seed=5)
    bg = torch.tensor(BACKGROUND_V1, device=device)
    dev = sc["means3d"].device
    _hip_mod.config_fused_sort(2)
    _fused._state.clear()
    for _ in range(3):
        img = ms.render_gaussians(*_g(sc), cam, background_color=bg, backend="hip", bin_size=bin_size)
        assert not _flags(dev) & FUSED_BIT
        _lane_back_to_default(dev)
    assert torch.equal(img, stagewise(sc, cam, bg, 16))
