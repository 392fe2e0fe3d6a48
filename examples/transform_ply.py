"""Move a 3DGS scene file in space: load -> transform_scene (x' = s R x + t, SH bands rotated with it) -> crop -> save.
The loader goes by the input file as in render_ply.py (``.splat``, a compressed ``.ply``, or the INRIA ``.ply``); the saver by
the output's name: ``*.splat`` -> save_splat, ``*.compressed.ply`` -> save_compressed_ply, any other name -> save_ply.

    python examples/transform_ply.py in.ply out.ply [--rotate-axis-angle X Y Z DEGREES] [--scale S] [--translate X Y Z]
                                     [--crop-box X0 Y0 Z0 X1 Y1 Z1] [--backend hip|torch]

The map is x' = S R x + T with R the rotation by DEGREES about the axis (X, Y, Z); --crop-box is applied AFTER the transform,
in the new coordinates (closed bounds).  COLMAP's y-down to a y-up viewer: --rotate-axis-angle 1 0 0 180.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mojosplat_amd import crop_scene, save_compressed_ply, save_ply, save_splat, transform_scene  # noqa: E402
from render_ply import loader_for  # noqa: E402


def saver_for(path):
    """The saver of the format the output's name asks for."""
    name = path.lower()
    if name.endswith(".splat"):
        return save_splat
    return save_compressed_ply if name.endswith(".compressed.ply") else save_ply


def axis_angle_matrix(axis, degrees):
    """Rodrigues' formula, float64: the rotation by `degrees` about `axis` (any non-zero length)."""
    a = torch.as_tensor(axis, dtype=torch.float64)
    if not float(a.norm()) > 0.0:
        raise SystemExit("--rotate-axis-angle: the axis must not be zero")
    x, y, z = (a / a.norm()).tolist()
    K = torch.tensor([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]], dtype=torch.float64)
    t = math.radians(degrees)
    return torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src", help="the scene to read (.ply, compressed .ply or .splat)")
    ap.add_argument("dst", help="the scene to write; the name picks the format")
    ap.add_argument("--rotate-axis-angle", type=float, nargs=4, metavar=("X", "Y", "Z", "DEGREES"))
    ap.add_argument("--translate", type=float, nargs=3, metavar=("X", "Y", "Z"))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--crop-box", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--backend", choices=("hip", "torch"), default="hip")
    args = ap.parse_args()
    if args.backend == "hip" and not torch.cuda.is_available():
        raise SystemExit("backend='hip' needs a ROCm GPU (--backend torch runs on the CPU)")
    p = loader_for(args.src)(args.src, backend=args.backend)
    N, K = p["features"].shape[:2]
    print(f"loaded {N} Gaussians, SH degree {math.isqrt(K) - 1}")
    rotation = None if args.rotate_axis_angle is None else axis_angle_matrix(args.rotate_axis_angle[:3], args.rotate_axis_angle[3])
    p = transform_scene(p, rotation=rotation, translation=args.translate, scale=args.scale, backend=args.backend)
    if args.crop_box is not None:
        p, keep = crop_scene(p, box=(args.crop_box[:3], args.crop_box[3:]))
        print(f"kept {int(keep.sum())} of {N} Gaussians")
        if not bool(keep.any()):
            raise SystemExit("--crop-box: no Gaussian is left")
    print(f"wrote {saver_for(args.dst)(args.dst, p, backend=args.backend)} bytes to {args.dst}")


if __name__ == "__main__":
    main()
