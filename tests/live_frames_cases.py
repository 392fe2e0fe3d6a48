"""Scenes and cameras for tests/test_hip_live_frames.py: several differentiable frames of ONE scene alive at once.

One scene (randscene_v1, N = 400: the size tests/test_hip_backward.py runs through the float64 restatement) seen by K = 3
cameras that must be told apart -- a backward that walked another live frame's records, lists or rows has to show: the
scene's own camera, a second one of the same 96 x 64 size from another eye (fx != fy, off-centre principal point), a third
one of 80 x 48 (another workspace layout, another tile grid).  Each view has its own cotangent and background.
test_the_cameras_can_be_told_apart (no GPU) holds the cameras to that.  OTHER_* is the
scene that runs BETWEEN the forwards and the backwards, STACK_* the frames whose sorted fronts run out (their backward's redo
launch writes the thread's pinned clean-up words)."""
import torch

from helpers import general_camera
from mojosplat_amd.scenes import randscene_v1

NAMES = ("means3d", "scales", "quats", "opacities", "features")
N, W, H, ELL, SEED = 400, 96, 64, -2.5, 11
K = 3
BACKGROUNDS = ((0.1, 0.1, 0.1), (0.3, 0.05, 0.2), (0.0, 0.25, 0.15))
BACKGROUNDS4 = tuple(b + (0.05 + 0.1 * k,) for k, b in enumerate(BACKGROUNDS))
MIN_VISIBLE = 0.25          # of the Gaussians, in every view
MIN_APART, APART_PX = 0.10, 8.0   # of the Gaussians visible in one view: culled in the other or further than this away
OTHER = dict(N=1200, W=160, H=100, ell=-3.0, seed=5)        # the inference scene between
OTHER_TRAIN = dict(N=3 * N, W=128, H=80, ell=-2.5, seed=6)  # the training scene between: 3N Gaussians, another resolution
STACK = (4000, 4.0, 6.0, 0.005)                              # test_hip_fused._stack_scene: every heavy bin's front runs out


def scene(device="cpu", channels=3):
    """-> dict(means3d, scales, quats, opacities, features (N, channels))."""
    return randscene_v1(N, W, H, ell=ELL, seed=SEED, device=device, channels=channels)[0]


def sh_coeffs(device="cpu"):
    """(N, 16, 3) coefficients of degree 3; some colours sit on the clamp at 0."""
    return (0.3 * torch.randn(N, 16, 3, generator=torch.Generator().manual_seed(4))).to(device)


def cameras(device="cpu"):
    """The K cameras: the scene's own; 96 x 64 from the right and below; 80 x 48 from the left, above and closer."""
    return [randscene_v1(1, W, H, ell=ELL, seed=SEED, device=device)[1],
            general_camera(W, H, 52.0, 41.0, 0.42 * W, 0.57 * H, near=0.1, far=100.0, eye=(4.2, -1.0, 2.6), target=(0.2, 0.1, -0.3),
                           device=device),
            general_camera(80, 48, 40.0, 46.0, 43.0, 22.0, near=0.1, far=100.0, eye=(-2.8, 2.2, -3.4), target=(-0.2, 0.0, 0.4),
                           device=device)]


def extra_camera(device="cpu"):
    """A fourth camera that renders nothing."""
    return general_camera(W, H, 30.0, 30.0, 0.5 * W, 0.5 * H, near=0.1, far=100.0, eye=(0.5, 3.0, 4.0), target=(0.0, 0.0, 0.0),
                          device=device)


def cotangents(device="cpu", channels=3):
    """One dL/dimage per view (seeded, drawn on the CPU)."""
    return [torch.rand(c.H, c.W, channels, generator=torch.Generator().manual_seed(43 + k)).to(device)
            for k, c in enumerate(cameras())]


def backgrounds(device="cpu", channels=3):
    return [torch.tensor(b, dtype=torch.float32, device=device) for b in (BACKGROUNDS if channels == 3 else BACKGROUNDS4)]


def targets(device="cpu"):
    """One target image per view for the photometric loss (seeded noise around mid grey: no exact ties with a render)."""
    return [(0.25 + 0.5 * torch.rand(c.H, c.W, 3, generator=torch.Generator().manual_seed(71 + k))).to(device)
            for k, c in enumerate(cameras())]


def other_scene(device="cpu", train=False):
    p = OTHER_TRAIN if train else OTHER
    return randscene_v1(p["N"], p["W"], p["H"], ell=p["ell"], seed=p["seed"], device=device)


def other_cameras(device="cpu"):
    """Two cameras of the inference scene's size for render_gaussians_batch."""
    p = OTHER
    f = 500.0 * p["W"] / 1920.0
    return [other_scene(device)[1],
            general_camera(p["W"], p["H"], f, f, p["W"] / 2.0, p["H"] / 2.0, near=0.1, far=100.0, eye=(2.0, 1.0, 4.5),
                           target=(0.0, 0.0, 0.0), device=device)]


def stack_cameras(device="cpu"):
    """_stack_scene's own camera and a second one of its size, turned about the pile's centre.

    Every entry of this scene sits by the alpha >= 1/255 test (opacities of 0.004 .. 0.006: a footprint ends where
    exp(-sigma) falls below ~0.78), some four million (pixel, Gaussian) pairs a frame.  The fused frame's backward evaluates
    alpha from the forward's records, the per-stage backward from the projected arrays: a pair within rounding of the
    threshold can be blended by one and skipped by the other, whatever else is alive.  An eye of (1.2, -0.7, 0.4) has such
    a pair in front of a pixel (Gaussian 2869, weight alpha T ~ 2.5e-4: its colour gradient moves by 7 %, the same for the
    frame alone and among others, and the forward disagrees with the float64 restatement at that pixel by 2.2e-4); this eye
    has none the STACKS bar would see, like the scene's own camera."""
    from test_hip_fused import _stack_scene
    cam = _stack_scene(1, *STACK[1:], device)[1]
    return [cam, general_camera(cam.W, cam.H, cam.fx, cam.fy, cam.cx, cam.cy, near=cam.near, far=cam.far, eye=(0.4, 0.2, 0.0),
                                target=(0.0, 0.0, 5.0), device=device)]


def told_apart(proj_a, proj_b):
    """Share of the Gaussians visible in view a that view b culls or puts more than APART_PX away.  proj_*: (means2d,
    conics, depths, radii) of oracle.project_fwd."""
    vis_a, vis_b = (proj_a[3] > 0).all(1), (proj_b[3] > 0).all(1)
    far = ((proj_a[0] - proj_b[0]) ** 2).sum(1) ** 0.5 > APART_PX
    return float((vis_a & (~vis_b | far)).sum()) / max(int(vis_a.sum()), 1)
