"""Forward + backward of the photometric loss on one GPU: the fused HIP kernels (photometric_loss, backend="hip")
against the same loss composed of torch ops -- what a user of the package had to run before -- alternated inside
one run, and the training step of scripts/bwd_probe.py's scene (config 3: randscene_v1, 1M Gaussians, 1920x1080) with
each of the two attached.  Writes profiles/loss_bench.json.  Fails without a GPU.

    python scripts/loss_bench.py [--reps 7] [--iters 50] [--no-step] [--out profiles/loss_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import mojosplat_amd as ms  # noqa: E402
from mojosplat_amd import _hip  # noqa: E402
from mojosplat_amd.autograd import render_gaussians_trainable  # noqa: E402
from mojosplat_amd.scenes import BACKGROUND_V1, randscene_v1  # noqa: E402

COPY_RATE, PEAK_RATE = 6.29e12, 8.0e12     # bytes/s: the measured copy rate and the HBM peak (MI355X_MICROARCH)
SIZES = [(1080, 1920, 3), (2160, 3840, 3)]


def make_torch_loss(device, C=3, lam=0.2):
    """The 3DGS loss as the trainers write it with torch ops on an (H, W, C) image: permute to NCHW, five depthwise
    conv2d with the 11x11 window (zero padding 5), the elementwise SSIM map, two means."""
    g = torch.tensor([math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float64)
    g = g / g.sum()
    window = (g[:, None] * g[None, :]).float().to(device).expand(C, 1, 11, 11).contiguous()
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    conv = lambda t: torch.nn.functional.conv2d(t, window, padding=5, groups=C)

    def loss_fn(img, target):
        x, y = img.permute(2, 0, 1)[None], target.permute(2, 0, 1)[None]
        mu_x, mu_y = conv(x), conv(y)
        mu_xx, mu_yy, mu_xy = mu_x * mu_x, mu_y * mu_y, mu_x * mu_y
        s_xx, s_yy, s_xy = conv(x * x) - mu_xx, conv(y * y) - mu_yy, conv(x * y) - mu_xy
        ssim_map = ((2 * mu_xy + C1) * (2 * s_xy + C2)) / ((mu_xx + mu_yy + C1) * (s_xx + s_yy + C2))
        return (1.0 - lam) * (img - target).abs().mean() + lam * (1.0 - ssim_map.mean())
    return loss_fn


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


def summary(ms_list):
    return dict(median_ms=round(statistics.median(ms_list), 5), min_ms=round(min(ms_list), 5), max_ms=round(max(ms_list), 5),
                spread_ms=round(max(ms_list) - min(ms_list), 5), reps=len(ms_list))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-step", action="store_true", help="skip the training step of config 3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench.py measures on a GPU: none is visible (no fallback)")
    dev = torch.device("cuda:0")
    _hip.lib()
    result = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "iters_per_rep": a.iters, "lambda_dssim": 0.2,
              "what": "forward + backward (dL/dimg) of the loss on a float32 (H, W, 3) image; ms per call between stream events, "
                      "hip and torch alternated rep by rep after warm-up of every shape", "sizes": {}}
    torch_loss = make_torch_loss(dev)
    for H, W, C in SIZES:
        gen = torch.Generator().manual_seed(H)
        img = torch.rand(H, W, C, generator=gen).to(dev).requires_grad_(True)
        target = torch.rand(H, W, C, generator=gen).to(dev)

        def run(loss_fn):
            img.grad = None
            loss_fn(img, target).backward()

        fns = {"hip": lambda: run(lambda x, y: ms.photometric_loss(x, y, backend="hip")),
               "torch_ops": lambda: run(torch_loss),
               "hip_forward_only": lambda: ms.ssim(img.detach(), target)}
        t = alternate(fns, a.reps, a.iters)
        n_bytes = 4 * H * W * C
        design_bytes = 11 * n_bytes        # forward 2 I in + 3 I of planes out, backward 5 I in + I out (csrc/loss.hip)
        hip, ref = summary(t["hip"]), summary(t["torch_ops"])
        spread = max(hip["spread_ms"], ref["spread_ms"])
        rate = design_bytes / (hip["median_ms"] * 1e-3)
        with torch.no_grad():
            lv = float(ms.photometric_loss(img, target)), float(torch_loss(img, target))
        result["sizes"][f"{W}x{H}x{C}"] = {
            "hip": hip, "torch_ops": ref, "hip_forward_only": summary(t["hip_forward_only"]),
            "ratio_torch_over_hip": round(ref["median_ms"] / hip["median_ms"], 3),
            "faster_by_more_than_the_spread": bool(ref["min_ms"] - hip["max_ms"] > 0 and ref["median_ms"] - hip["median_ms"] > spread),
            "design_bytes_per_step": design_bytes, "achieved_bytes_per_s": round(rate, 1),
            "share_of_copy_rate_6.29TBs": round(rate / COPY_RATE, 4), "share_of_peak_8TBs": round(rate / PEAK_RATE, 4),
            "loss_hip": lv[0], "loss_torch_ops": lv[1]}
        print(json.dumps({f"{W}x{H}x{C}": result["sizes"][f"{W}x{H}x{C}"]}), flush=True)
        del img, target
        torch.cuda.empty_cache()

    if not a.no_step:
        N, W, H = 1_000_000, 1920, 1080
        sc, cam = randscene_v1(N, W, H, ell=-4.0, seed=42, device=dev)
        bg = torch.tensor(BACKGROUND_V1, device=dev)
        leaves = [sc[k].float().clone().requires_grad_(True) for k in ("means3d", "scales", "quats", "opacities", "features")]
        target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(43)).to(dev)
        v_img = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(44)).to(dev)

        def step(loss_fn):
            for l in leaves:
                l.grad = None
            out = render_gaussians_trainable(*leaves, cam, background_color=bg)
            if loss_fn is None:
                out.backward(v_img)
            else:
                loss_fn(out, target).backward()

        fns = {"render_only": lambda: step(None),
               "with_hip_loss": lambda: step(lambda x, y: ms.photometric_loss(x, y, backend="hip")),
               "with_torch_ops_loss": lambda: step(torch_loss)}
        t = alternate(fns, a.reps, max(10, a.iters // 2))
        result["training_step_cfg3"] = {"what": "render_gaussians_trainable (randscene_v1, 1M Gaussians, 1920x1080) + loss + backward to "
                                                "the five leaves, streamed (no host wait inside a rep); render_only: dL/dimg given",
                                        **{k: summary(v) for k, v in t.items()}}
        print(json.dumps({"training_step_cfg3": result["training_step_cfg3"]}), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
