"""Prune a 3DGS scene file by what its Gaussians contribute to images: load -> accumulate_contributions over a set of views
-> select_by_contribution -> prune_scene -> save.  The loader goes by the input file as in render_ply.py (``.splat``, a
compressed ``.ply``, or the INRIA ``.ply``); the output is written in the input's format.

    python examples/prune_ply.py in.ply out.ply [--min-max-weight 0.01] [--keep-fraction 0.5] [--views 24] [--width 640]
                                 [--height 480] [--distance 2.5] [--view EX EY EZ TX TY TZ ...] [--backend hip|torch]

--min-max-weight TAU keeps a Gaussian whose blend weight alpha * T reaches TAU on some pixel of some view (RadSplat's rule),
--keep-fraction F the ceil(F N) largest by summed blend weight (LightGaussian's score without its volume term); both: the AND.
The views are a ring of --views cameras on the scene's bounding sphere, --distance radii from its centre, looking at the
centre, at three heights; every --view adds a camera at eye (EX, EY, EZ) looking at (TX, TY, TZ), and with --views 0 only
those are used.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mojosplat_amd import (Camera, ContributionStats, accumulate_contributions, load_compressed_ply, load_splat, look_at,  # noqa: E402
                           prune_scene, save_compressed_ply, save_ply, save_splat, select_by_contribution)
from render_ply import loader_for  # noqa: E402


def saver_like(loader):
    """The saver of the format that `loader` reads."""
    return {load_splat: save_splat, load_compressed_ply: save_compressed_ply}.get(loader, save_ply)


def bounding_sphere(means3d):
    """-> (centre (3,) float32 on the CPU, radius): the mean and the largest distance from it (1 for a single point)."""
    m = means3d.detach().float().cpu()
    centre = m.mean(0)
    return centre, float((m - centre).norm(dim=-1).max()) or 1.0


def camera_at(eye, target, W, H, radius, dev):
    """A pinhole camera (60 degrees across) at `eye` looking at `target`."""
    eye, target = torch.as_tensor(eye, dtype=torch.float32), torch.as_tensor(target, dtype=torch.float32)
    forward = target - eye
    up = torch.tensor([0.0, 1.0, 0.0])
    if float(torch.linalg.cross(forward, up).norm()) < 1e-6 * float(forward.norm()):
        up = torch.tensor([0.0, 0.0, 1.0])        # looking straight up or down
    vm = look_at(eye, target, up)
    f = 0.5 * W / math.tan(math.radians(30.0))
    return Camera(R=vm[:3, :3].contiguous().to(dev), T=vm[:3, 3].contiguous().to(dev), H=H, W=W, fx=f, fy=f, cx=W / 2.0,
                  cy=H / 2.0, near=0.01 * radius, far=100.0 * radius)


def ring_cameras(centre, radius, n, distance, W, H, dev):
    """`n` cameras around the sphere, `distance` radii from its centre, at elevations -20, 10 and 40 degrees in turn."""
    cams = []
    for i in range(n):
        az, el = 2.0 * math.pi * i / n, math.radians((-20.0, 10.0, 40.0)[i % 3])
        d = torch.tensor([math.cos(el) * math.sin(az), math.sin(el), math.cos(el) * math.cos(az)])
        cams.append(camera_at(centre + d * radius * distance, centre, W, H, radius, dev))
    return cams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src", help="the scene to read (.ply, compressed .ply or .splat)")
    ap.add_argument("dst", help="the scene to write, in the input's format")
    ap.add_argument("--min-max-weight", type=float, default=None)
    ap.add_argument("--keep-fraction", type=float, default=None)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--view", type=float, nargs=6, action="append", default=[], metavar=("EX", "EY", "EZ", "TX", "TY", "TZ"))
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--distance", type=float, default=2.5)
    ap.add_argument("--backend", choices=("hip", "torch"), default="hip")
    args = ap.parse_args()
    if args.min_max_weight is None and args.keep_fraction is None:
        raise SystemExit("give --min-max-weight, --keep-fraction or both")
    if args.views <= 0 and not args.view:
        raise SystemExit("no views: give --views N or at least one --view")
    if args.backend == "hip" and not torch.cuda.is_available():
        raise SystemExit("backend='hip' needs a ROCm GPU (--backend torch runs on the CPU)")
    loader = loader_for(args.src)
    p = loader(args.src, backend=args.backend)
    N, dev = p["means3d"].shape[0], p["means3d"].device
    centre, radius = bounding_sphere(p["means3d"])
    cams = ring_cameras(centre, radius, max(args.views, 0), args.distance, args.width, args.height, dev)
    cams += [camera_at(v[:3], v[3:], args.width, args.height, radius, dev) for v in args.view]
    print(f"loaded {N} Gaussians; {len(cams)} views of {args.width}x{args.height}")
    stats = ContributionStats(N, dev)
    opacities = torch.sigmoid(p["opacities"])
    for cam in cams:
        accumulate_contributions(stats, p["means3d"], p["scales"], p["quats"], opacities, cam, backend=args.backend)
    keep = select_by_contribution(stats, min_max_weight=args.min_max_weight, keep_fraction=args.keep_fraction)
    kept = int(keep.sum())
    print(f"never blended: {int((stats.pixels == 0).sum())}; kept {kept} of {N} Gaussians")
    if kept == 0:
        raise SystemExit("no Gaussian is left")
    p = prune_scene(p, keep)
    print(f"wrote {saver_like(loader)(args.dst, p, backend=args.backend)} bytes to {args.dst}")


if __name__ == "__main__":
    main()
