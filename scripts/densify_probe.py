"""Cost of the densification statistics on the training step (GPU): config 3 (randscene-v1, 1M Gaussians, 1920x1080),
render_gaussians_trainable + backward with densify=DensifyStats and without, alternated in blocks within one process.

    python scripts/densify_probe.py [--steps 200] [--block 20] [--out densify_probe.json]

streamed: a block of steps launched back to back, timed by two events (mean per step); synchronised: each step timed
alone between two events after a device sync.  Medians over the blocks / steps of each setting.  The kernel times
(k_project_ewa_bwd<2, true> against <2>) come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mojosplat_amd.autograd import render_gaussians_trainable  # noqa: E402
from mojosplat_amd.densify import DensifyStats  # noqa: E402
from mojosplat_amd.scenes import BACKGROUND_V1, randscene_v1  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps of each setting, streamed and synchronised each")
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, W, H = 1_000_000, 1920, 1080
    sc, cam = randscene_v1(N, W, H, ell=-4.0, seed=42, device=dev)
    bg = torch.tensor(BACKGROUND_V1, device=dev)
    leaves = [sc[k].clone().requires_grad_(True) for k in ("means3d", "scales", "quats", "opacities", "features")]
    v_img = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    stats = DensifyStats(N, dev)

    def step(on):
        for l in leaves:
            l.grad = None
        img = render_gaussians_trainable(*leaves, cam, background_color=bg, densify=stats if on else None)
        (img * v_img).sum().backward()

    for _ in range(a.warmup):
        step(False), step(True)
    torch.cuda.synchronize()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    streamed = {False: [], True: []}
    synced = {False: [], True: []}
    blocks = max(1, a.steps // a.block)
    for b in range(2 * blocks):
        on = bool(b % 2)
        e0, e1 = ev(), ev()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.block):
            step(on)
        e1.record()
        torch.cuda.synchronize()
        streamed[on].append(e0.elapsed_time(e1) * 1e3 / a.block)
        for _ in range(a.block):
            e0, e1 = ev(), ev()
            torch.cuda.synchronize()
            e0.record()
            step(on)
            e1.record()
            torch.cuda.synchronize()
            synced[on].append(e0.elapsed_time(e1) * 1e3)
    med = lambda xs: statistics.median(xs)
    res = {
        "workload": f"cfg3: randscene-v1 N={N} {W}x{H} ell=-4.0 seed=42, render_gaussians_trainable + backward",
        "steps_per_setting": {"streamed": blocks * a.block, "synchronised": len(synced[True])},
        "streamed_us_per_step": {"off": med(streamed[False]), "on": med(streamed[True])},
        "synchronised_us_per_step": {"off": med(synced[False]), "on": med(synced[True])},
    }
    res["streamed_delta_us"] = res["streamed_us_per_step"]["on"] - res["streamed_us_per_step"]["off"]
    res["synchronised_delta_us"] = res["synchronised_us_per_step"]["on"] - res["synchronised_us_per_step"]["off"]
    res["stats_count_sum"] = float(stats.count.sum())
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
