"""Bilateral-grid colour correction on one GPU: the fused HIP kernels (bilagrid_slice / bilagrid_tv_loss, backend="hip")
against their torch definitions (backend="torch": explicit gathers, autograd) alternated inside one run.  Times the slice
forward + backward (both gradients) at 1920x1080x3 under a 16x16x8 grid for B = 1, and the TV loss forward + backward for
1 and for 200 views.  Writes profiles/bilagrid_bench.json.  Fails without a GPU.  Nothing here asserts a time or a ratio.

    python scripts/bilagrid_bench.py [--reps 7] [--iters 50] [--out profiles/bilagrid_bench.json]
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

COPY_RATE = 6.29e12     # bytes/s: the copy rate the project quotes for an MI355X
H, W, GRID = 1080, 1920, (16, 16, 8)


def timed(fn, iters):
    """ms per call of fn between two stream events around `iters` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, reps, iters, warm=5):
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


def streamed(fn, reps, iters, device):
    """[ms per call] * reps with the host running ahead of the device: about 10 ms of matrix products are queued in front
    of the timed calls, so the span between the two events is the device's time for them, not the host's time to launch
    them (a training loop queues a render and a loss around these calls in the same way)."""
    a = torch.randn(8192, 8192, device=device)
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        for _ in range(8):
            a @ a
        out.append(timed(fn, iters))
    return out


def summary(ms_list):
    return dict(median_ms=round(statistics.median(ms_list), 5), min_ms=round(min(ms_list), 5), max_ms=round(max(ms_list), 5),
                spread_ms=round(max(ms_list) - min(ms_list), 5), reps=len(ms_list))


def entry(t, design_bytes):
    """bytes/s on the design bytes over the device's own time (hip_streamed); hip: what a lone call costs from the host."""
    hip, ref, dev = summary(t["hip"]), summary(t["torch"]), summary(t["hip_streamed"])
    rate = design_bytes / (dev["median_ms"] * 1e-3)
    out = {"hip": hip, "torch": ref, "ratio_torch_over_hip": round(ref["median_ms"] / hip["median_ms"], 3),
           "ratio_torch_over_hip_streamed": round(ref["median_ms"] / dev["median_ms"], 3),
           "design_bytes": design_bytes, "achieved_bytes_per_s": round(rate, 1),
           "share_of_copy_rate_6.29TBs": round(rate / COPY_RATE, 4)}
    out.update({k: summary(v) for k, v in t.items() if k not in ("hip", "torch")})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilagrid_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bilagrid_bench.py measures on a GPU: none is visible (no fallback)")
    dev = torch.device("cuda:0")
    _hip.lib()
    result = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "iters_per_rep": a.iters,
              "what": "ms per call between stream events, hip and the torch definition alternated rep by rep after warm-up; "
                      "*_streamed: the same calls queued behind about 10 ms of matrix products, so that the host runs ahead and "
                      "the events span the device's own time; "
                      "design bytes: the slice reads img and writes out (2 I), its backward reads img and v_out and writes v_img "
                      "(3 I; the gather's re-reads of img and v_out are meant to hit L2), I = 12 B H W; the TV loss reads the "
                      "grids forward and reads and writes them backward (3 G)"}
    gen = torch.Generator().manual_seed(0)
    grids = (ms.bilagrid_identity(1, GRID, requires_grad=False) + 0.3 * torch.randn(1, 12, GRID[2], GRID[1], GRID[0], generator=gen))
    grids = grids.to(dev).requires_grad_(True)
    img = (torch.rand(1, H, W, 3, generator=gen) * 1.4 - 0.2).to(dev).requires_grad_(True)
    v_out = torch.randn(1, H, W, 3, generator=gen).to(dev)

    def slice_step(backend):
        grids.grad = img.grad = None
        ms.bilagrid_slice(grids, img, backend=backend).backward(v_out)

    def slice_forward():
        with torch.no_grad():
            ms.bilagrid_slice(grids, img)

    def slice_image_gradient_only():
        img.grad = None
        ms.bilagrid_slice(grids.detach(), img).backward(v_out)

    t = alternate({"hip": lambda: slice_step("hip"), "torch": lambda: slice_step("torch"), "hip_forward_only": slice_forward,
                   "hip_forward_and_v_img_only": slice_image_gradient_only}, a.reps, a.iters)
    t["hip_streamed"] = streamed(lambda: slice_step("hip"), a.reps, a.iters, dev)
    t["hip_forward_only_streamed"] = streamed(slice_forward, a.reps, a.iters, dev)
    result[f"slice_fwd_bwd_{W}x{H}x3_grid{GRID[0]}x{GRID[1]}x{GRID[2]}_B1"] = entry(t, 5 * 12 * H * W)
    print(json.dumps(result), flush=True)
    del img, v_out
    torch.cuda.empty_cache()

    for B in (1, 200):
        g = (ms.bilagrid_identity(B, GRID, requires_grad=False) + 0.3 * torch.randn(B, 12, GRID[2], GRID[1], GRID[0], generator=gen))
        g = g.to(dev).requires_grad_(True)

        def tv_step(backend):
            g.grad = None
            ms.bilagrid_tv_loss(g, backend=backend).backward()

        t = alternate({"hip": lambda: tv_step("hip"), "torch": lambda: tv_step("torch")}, a.reps, a.iters)
        t["hip_streamed"] = streamed(lambda: tv_step("hip"), a.reps, a.iters, dev)
        key = f"tv_fwd_bwd_B{B}_grid{GRID[0]}x{GRID[1]}x{GRID[2]}"
        result[key] = entry(t, 3 * 4 * g.numel())
        print(json.dumps({key: result[key]}), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
