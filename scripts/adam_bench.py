"""The optimiser step of 3DGS training on one GPU: GaussianAdam (backend="hip": one launch of csrc/adam.hip for the five
tensors of a scene), dense and under visibility masks, against torch.optim.Adam with default flags and with fused=True --
alternated inside one run -- on 1 M Gaussians with (a) RGB colours, 14 floats per Gaussian, and (b) SH degree 3, 59
floats; and the training step of config 3 (randscene_v1, 1 M Gaussians, 1920x1080: render, loss, backward, optimiser)
with each optimiser attached.  Writes profiles/adam_bench.json.  Fails without a GPU.

    python scripts/adam_bench.py [--reps 7] [--iters 30] [--no-step] [--out profiles/adam_bench.json]
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
from mojosplat_amd import GaussianAdam, _hip  # noqa: E402
from mojosplat_amd.autograd import render_gaussians_trainable  # noqa: E402
from mojosplat_amd.scenes import BACKGROUND_V1, randscene_v1  # noqa: E402

COPY_RATE = 6.29e12                    # bytes/s: the copy rate DESIGN.md measured
BYTES_PER_ELEMENT = 28                 # p, g, m, v in; p, m, v out
NAMES = ("means3d", "scales", "quats", "opacities", "features")
LRS = {"means3d": 1.6e-4, "scales": 5e-3, "quats": 1e-3, "opacities": 5e-2, "features": 2.5e-3}
N, W, H = 1_000_000, 1920, 1080


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


def summary(ms_list, elements=None):
    s = dict(median_ms=round(statistics.median(ms_list), 5), min_ms=round(min(ms_list), 5), max_ms=round(max(ms_list), 5),
             spread_ms=round(max(ms_list) - min(ms_list), 5), reps=len(ms_list))
    if elements is not None:
        rate = BYTES_PER_ELEMENT * elements / (s["median_ms"] * 1e-3)
        s.update(elements_updated=int(elements), bytes_on_28_per_element=int(BYTES_PER_ELEMENT * elements),
                 achieved_bytes_per_s=round(rate, 1), share_of_copy_rate_6_29TBs=round(rate / COPY_RATE, 4))
    return s


def masks_of(n, view_mask, dev):
    """{name: (N,) bool}: 100 / 30 / 10 % of the rows as one contiguous run, the same shares scattered at random, the view's."""
    out = {}
    r = torch.rand(n, generator=torch.Generator().manual_seed(7)).to(dev)
    for share in (100, 30, 10):
        m = torch.zeros(n, dtype=torch.bool, device=dev)
        m[n // 5: n // 5 + n * share // 100] = True
        if share == 100:
            m[:] = True
        out[f"contiguous_{share}"] = m
    for share in (100, 30, 10):
        out[f"scattered_{share}"] = r < share / 100.0
    out["view_morton"] = view_mask
    return out


def bench_optimisers(label, feature_shape, scene_sorted, view_mask, a, dev):
    gen = torch.Generator().manual_seed(11)
    shapes = {"means3d": (N, 3), "scales": (N, 3), "quats": (N, 4), "opacities": (N,), "features": (N, *feature_shape)}
    params = {k: (scene_sorted[k] if scene_sorted[k].shape == s else torch.rand(s, generator=gen).to(dev)).clone().requires_grad_(True)
              for k, s in shapes.items()}
    for p in params.values():
        p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(dev)
    elements = sum(p.numel() for p in params.values())
    groups = lambda: [{"params": [params[k]], "lr": LRS[k]} for k in NAMES]     # (Adam writes its defaults into them)
    opts = {"torch_adam": torch.optim.Adam(groups(), eps=1e-15),
            "torch_adam_fused": torch.optim.Adam(groups(), eps=1e-15, fused=True)}
    hip = GaussianAdam(params, lr=LRS, eps=1e-15, backend="hip")
    masks = masks_of(N, view_mask, dev)
    fns = {k: o.step for k, o in opts.items()}
    fns["gaussian_adam_dense"] = hip.step
    for k, m in masks.items():
        fns[f"gaussian_adam_mask_{k}"] = (lambda m=m: hip.step(visibility=m))
    t = alternate(fns, a.reps, a.iters)
    width = elements // N
    res = {"floats_per_gaussian": width, "elements": elements}
    for k, v in t.items():
        share = float(masks[k[len("gaussian_adam_mask_"):]].float().mean()) if k.startswith("gaussian_adam_mask_") else 1.0
        res[k] = summary(v, elements=round(share * N) * width)
        if share != 1.0 or k.startswith("gaussian_adam_mask_"):
            res[k]["visible_share"] = round(share, 4)
    d, f = res["gaussian_adam_dense"], res["torch_adam_fused"]
    res["dense_vs_fused"] = {"ratio_fused_over_hip": round(f["median_ms"] / d["median_ms"], 3),
                             "hip_faster_by_more_than_the_spread": bool(f["min_ms"] - d["max_ms"] > 0 and
                                                                        f["median_ms"] - d["median_ms"] > max(f["spread_ms"], d["spread_ms"]))}
    res["dense_bound_ms_at_copy_rate"] = round(BYTES_PER_ELEMENT * elements / COPY_RATE * 1e3, 5)
    print(json.dumps({label: res}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-step", action="store_true", help="skip the training step of config 3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_bench.py measures on a GPU: none is visible (no fallback)")
    dev = torch.device("cuda:0")
    _hip.lib()
    result = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "iters_per_rep": a.iters, "gaussians": N,
              "what": "one optimiser step over the five tensors of a scene (float32); ms per step between stream events, all "
                      "variants alternated rep by rep after warm-up; bytes: 28 per updated element (p, g, m, v in; p, m, v "
                      "out) -- for a masked step the elements of its visible rows -- against the 6.29 TB/s copy rate"}
    sc, cam = randscene_v1(N, W, H, ell=-4.0, seed=42, device=dev)
    prepared = ms.prepare_scene(*[sc[k] for k in NAMES])
    sorted_scene = dict(zip(NAMES, prepared.arrays))
    radii = ms.project_gaussians(*[sorted_scene[k] for k in NAMES[:4]], cam, backend="hip")[3]
    view_mask = (radii > 0).all(-1).contiguous()
    result["view_mask"] = {"what": "radii > 0 of project_gaussians(backend='hip') for randscene_v1's camera on the scene in "
                                   "prepare_scene's Morton order", "visible_share": round(float(view_mask.float().mean()), 4)}
    result["rgb"] = bench_optimisers("rgb", (3,), sorted_scene, view_mask, a, dev)
    torch.cuda.empty_cache()
    result["sh3"] = bench_optimisers("sh3", (16, 3), sorted_scene, view_mask, a, dev)
    torch.cuda.empty_cache()

    if not a.no_step:
        bg = torch.tensor(BACKGROUND_V1, device=dev)
        leaves = {k: sorted_scene[k].float().clone().requires_grad_(True) for k in NAMES}
        target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(43)).to(dev)
        tiny = {k: 1e-9 for k in NAMES}          # the scene stays what it is over the run: every variant times the same frame
        groups = lambda: [{"params": [leaves[k]], "lr": tiny[k]} for k in NAMES]
        adam = torch.optim.Adam(groups(), eps=1e-15)
        fused = torch.optim.Adam(groups(), eps=1e-15, fused=True)
        hip = GaussianAdam(leaves, lr=tiny, eps=1e-15, backend="hip")

        def step(update):
            for l in leaves.values():
                l.grad = None
            img = render_gaussians_trainable(*[leaves[k] for k in NAMES], cam, background_color=bg)
            ms.photometric_loss(img, target, backend="hip").backward()
            if update is not None:
                update()

        fns = {"no_optimiser": lambda: step(None), "torch_adam": lambda: step(adam.step),
               "torch_adam_fused": lambda: step(fused.step), "gaussian_adam_dense": lambda: step(hip.step),
               "gaussian_adam_mask_view_morton": lambda: step(lambda: hip.step(visibility=view_mask))}
        t = alternate(fns, a.reps, max(10, a.iters // 2))
        result["training_step_cfg3"] = {"what": "render_gaussians_trainable (randscene_v1 in Morton order, 1M Gaussians, RGB, 1920x1080) + "
                                                "photometric_loss (hip) + backward + the optimiser's step, streamed (no host wait inside "
                                                "a rep); the mask is computed once, outside the step", **{k: summary(v) for k, v in t.items()}}
        print(json.dumps({"training_step_cfg3": result["training_step_cfg3"]}), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
