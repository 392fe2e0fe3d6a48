"""Render a 3DGS scene file on the HIP backend: load -> evaluate_sh -> render_gaussians -> PNG (PIL if available, else .ppm).
The loader goes by the file: ``.splat`` -> load_splat; ``.ply`` whose header has ``element chunk`` -> load_compressed_ply (the
PlayCanvas / SuperSplat compressed PLY: mojosplat_amd/splatio.py); any other ``.ply`` -> load_ply (the INRIA point_cloud.ply
layout: mojosplat_amd/sceneio.py).  The camera looks at the scene's centre from outside it.

    python examples/render_ply.py scene.ply [--sh-degree 3] [--width 1280] [--height 720] [--distance 2.5] [--out output/render_ply.png]

--sh-degree defaults to the degree the file holds; a lower one evaluates only the leading coefficients.  Without a file,
--demo N writes N random Gaussians (init_from_points, degree 3) to a temporary scene first, so that the example runs on its own.
"""
import argparse
import math
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojosplat_amd import (Camera, evaluate_sh, init_from_points, load_compressed_ply, load_ply, load_splat, look_at,  # noqa: E402
                           render_gaussians, save_ply)
from render_sample import save_image  # noqa: E402


def loader_for(path):
    """The loader of the file's format: by extension and, for ``.ply``, by whether the header has ``element chunk``."""
    if path.lower().endswith(".splat"):
        return load_splat
    with open(path, "rb") as f:
        head = f.read(1 << 16)
    end = head.find(b"end_header")
    return load_compressed_ply if b"element chunk" in (head if end < 0 else head[:end]) else load_ply


def camera_for(means3d, W, H, distance, dev):
    """A pinhole camera (60 degrees across) on the +z side of the scene, `distance` scene radii from its centre."""
    centre = means3d.mean(0).cpu()
    radius = float((means3d.cpu() - centre).norm(dim=-1).quantile(0.9)) or 1.0
    eye = centre + torch.tensor([0.0, 0.3, 1.0]) * radius * distance
    vm = look_at(eye, centre, torch.tensor([0.0, 1.0, 0.0]))
    f = 0.5 * W / math.tan(math.radians(30.0))
    return Camera(R=vm[:3, :3].contiguous().to(dev), T=vm[:3, 3].contiguous().to(dev), H=H, W=W, fx=f, fy=f, cx=W / 2.0,
                  cy=H / 2.0, near=0.01 * radius, far=100.0 * radius)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ply", nargs="?", help="the scene (.ply, compressed .ply or .splat); omit it with --demo")
    ap.add_argument("--demo", type=int, default=0, help="write this many random Gaussians to a temporary scene and render that")
    ap.add_argument("--sh-degree", type=int, default=None)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--distance", type=float, default=2.5)
    ap.add_argument("--out", default="output/render_ply.png")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("backend='hip' needs a ROCm GPU")
    if not args.ply and args.demo <= 0:
        raise SystemExit("give a .ply file, or --demo N")
    dev = torch.device("cuda:0")
    tmp = None
    if not args.ply:
        g = torch.Generator().manual_seed(42)
        p = init_from_points(torch.randn((args.demo, 3), generator=g).to(dev), torch.rand((args.demo, 3), generator=g).to(dev),
                             sh_degree=3, init_opacity=0.6, requires_grad=False)
        p["features"][:, 1:] = 0.05 * torch.randn((args.demo, 15, 3), generator=g).to(dev)
        tmp = tempfile.TemporaryDirectory()
        args.ply = os.path.join(tmp.name, "demo.ply")
        print(f"wrote {save_ply(args.ply, p)} bytes to {args.ply}")
    t0 = time.perf_counter()
    p = loader_for(args.ply)(args.ply, device=dev)
    N, K = p["features"].shape[:2]
    file_degree = math.isqrt(K) - 1
    degree = file_degree if args.sh_degree is None else args.sh_degree
    if not 0 <= degree <= file_degree:
        raise SystemExit(f"--sh-degree {degree}: the file holds degree {file_degree}")
    print(f"loaded {N} Gaussians, SH degree {file_degree}, in {(time.perf_counter() - t0) * 1e3:.1f} ms")
    cam = camera_for(p["means3d"], args.width, args.height, args.distance, dev)
    colours = evaluate_sh(p["means3d"], p["features"][:, :(degree + 1) ** 2].contiguous(), cam, degree)
    img = render_gaussians(p["means3d"], p["scales"], p["quats"], torch.sigmoid(p["opacities"]), colours, cam,
                           background_color=torch.zeros(3, device=dev), backend="hip")
    torch.cuda.synchronize()
    print(f"rendered {tuple(img.shape)}, range [{img.min().item():.4f}, {img.max().item():.4f}]")
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    print("saved", save_image((img.clamp(0, 1).cpu().numpy() * 255).astype("uint8"), args.out))
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
