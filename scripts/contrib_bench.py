"""Contribution statistics of one view on one GPU, at the scale of the flagship benchmark: 1 M Gaussians (randscene_v1, the
scene of bench.py and the other benches) at 1920x1080.  Per view it times, alternated inside one run:

  accumulate        accumulate_contributions(backend="hip") with a weight map: project + bin (with its one host read) + the
                    ms_contrib_accumulate launch
  kernel            contributions_from_lists(backend="hip") on lists made once: the launch alone, with and without weights
  gradient_route    the only route to the weighted sum without this kernel: render_gaussians_trainable forward + backward
                    under L = sum_p weights_p img[p, 0], read off channel 0 of dL/dcolours

and records the two results' agreement.  Writes profiles/contrib_bench.json.  Fails without a GPU.  Nothing here asserts a
time or a ratio.

    python scripts/contrib_bench.py [--reps 7] [--iters 20] [--n 1000000] [--out profiles/contrib_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import mojosplat_amd as ms  # noqa: E402
from mojosplat_amd import _hip  # noqa: E402
from mojosplat_amd.autograd import render_gaussians_trainable  # noqa: E402
from mojosplat_amd.binning import bin_gaussians_to_tiles_hip  # noqa: E402
from mojosplat_amd.projection import project_gaussians_hip  # noqa: E402
from mojosplat_amd.scenes import randscene_v1  # noqa: E402

H, W, TILE = 1080, 1920, 16


def timed(fn, iters):
    """ms per call of fn between two stream events around `iters` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, reps, iters, warm=3):
    """{name: [ms per call] * reps}: every fn warmed, then the fns alternated rep by rep."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(timed(fn, iters))
    return out


def summary(ms_list):
    return dict(median_ms=round(statistics.median(ms_list), 5), min_ms=round(min(ms_list), 5), max_ms=round(max(ms_list), 5),
                spread_ms=round(max(ms_list) - min(ms_list), 5), reps=len(ms_list))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrib_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrib_bench.py measures on a GPU: none is visible (no fallback)")
    dev = torch.device("cuda:0")
    _hip.lib()
    scene, cam = randscene_v1(a.n, W, H, device=dev)
    m, s, q, o = (scene[k] for k in ("means3d", "scales", "quats", "opacities"))
    wmap = torch.rand(H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    stats = ms.ContributionStats(a.n, dev)
    m2, con, depths, radii = project_gaussians_hip(m, s, q, o, cam)
    ids, ranges = bin_gaussians_to_tiles_hip(m2, radii, depths, TILE, -(-W // TILE), -(-H // TILE))
    M = ids.numel()
    colours = scene["features"].clone().requires_grad_(True)

    def gradient_route():
        colours.grad = None
        img = render_gaussians_trainable(m, s, q, o, colours, cam, background_color=None, tile_size=TILE)
        (wmap * img[..., 0]).sum().backward()

    t = alternate({
        "accumulate": lambda: ms.accumulate_contributions(stats, m, s, q, o, cam, weights=wmap, tile_size=TILE),
        "kernel": lambda: ms.contributions_from_lists(stats, m2, con, o, ranges, ids, cam, weights=wmap, tile_size=TILE),
        "kernel_no_weights": lambda: ms.contributions_from_lists(stats, m2, con, o, ranges, ids, cam, tile_size=TILE),
        "gradient_route": gradient_route}, a.reps, a.iters)

    stats.reset()
    ms.contributions_from_lists(stats, m2, con, o, ranges, ids, cam, weights=wmap, tile_size=TILE)
    gradient_route()
    torch.cuda.synchronize()
    got, want = stats.weighted_sum(), colours.grad[:, 0].double()
    result = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "iters_per_rep": a.iters, "N": a.n, "W": W, "H": H,
              "tile_size": TILE, "M_list_entries": M,
              "what": "ms per call between stream events, the four alternated rep by rep after warm-up; accumulate includes "
                      "binning's one host read; design bytes of the kernel: 4 + 24 per list entry read, plus up to four "
                      "atomics per blended (block, entry)",
              "design_bytes_read": 28 * M,
              "blended_gaussians": int((stats.pixels > 0).sum()), "blended_pixel_pairs": int(stats.pixels.sum()),
              "max_abs_difference_weighted_sum_vs_gradient": float((got - want).abs().max()),
              "largest_weighted_sum": float(got.max()),
              "per_view": {k: summary(v) for k, v in t.items()}}
    med = {k: v["median_ms"] for k, v in result["per_view"].items()}
    result["ratio_gradient_route_over_accumulate"] = round(med["gradient_route"] / med["accumulate"], 3)
    result["ratio_gradient_route_over_kernel"] = round(med["gradient_route"] / med["kernel"], 3)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
