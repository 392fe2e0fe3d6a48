"""The scene transform on one GPU (mojosplat_amd/edit.py): one call of ms_scene_transform (csrc/transform.hip) against the
torch definition of the same step on the same GPU and inputs, at 1 M Gaussians with K = 1 and K = 16 (SH degree 3); and, for
one seeded scene of mojosplat_amd/scenes.py at a golden's size (5000 Gaussians, 640 x 360) given degree-3 SH colours, the PSNR
of the frame of the transformed scene under the transformed camera against the frame of the scene itself, for s = 1 and
s = 2.  The PSNRs are recorded, not asserted.  Writes profiles/transform_bench.json.  Fails without a GPU.

    python scripts/transform_bench.py [--n 1000000] [--reps 7] [--iters 5] [--limit 120] [--out profiles/transform_bench.json]

Byte model: 4 (11 + 3 K) bytes read and as many written per Gaussian (means, log-scales, quaternions, features; the opacities
are torch's clone on both backends and are not timed).  The share of the copy rate is that over the measured 6.29 TB/s of a
float4 copy.  Every timed step runs under its own time limit (--limit seconds, checked between calls).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from mojosplat_amd import _hip, edit, render_gaussians, transform_camera, transform_scene  # noqa: E402
from mojosplat_amd.knn import SH_C0  # noqa: E402
from mojosplat_amd.scenes import randscene_v1  # noqa: E402
from mojosplat_amd.sceneio import TENSORS  # noqa: E402

COPY_RATE = 6.29e12           # bytes/s, the measured float4 copy rate of the MI355X
ROTATION = [[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]]      # a rotation with exact decimal entries
TRANSLATION = [0.5, -1.25, 2.0]


class StepTimeout(RuntimeError):
    pass


def scene(N, K, dev):
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(s, generator=g).to(dev)
    return {"means3d": r(N, 3), "scales": r(N, 3) - 4.0, "quats": r(N, 4), "opacities": r(N), "features": r(N, K, 3)}


def timed_events(fn, iters):
    """Milliseconds per call between two device events around `iters` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}


def interleaved(calls, reps, iters, limit):
    """Each call in turn, `reps` rounds (the variants alternate inside one process); a step that passes `limit` seconds stops."""
    times = {name: [] for name in calls}
    for name, fn in calls.items():
        t0 = time.perf_counter()
        for _ in range(3):                                           # warm-up: code objects, allocator
            fn()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 > limit:
            raise StepTimeout(f"{name}: warm-up took more than {limit} s")
    for _ in range(reps):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            times[name].append(timed_events(fn, iters))
            if time.perf_counter() - t0 > limit:
                raise StepTimeout(f"{name}: one timed step took more than {limit} s")
    return {name: stats(v) for name, v in times.items()}


def bench(N, K, dev, a):
    p = scene(N, K, dev)
    t = [p[k] for k in TENSORS]
    s, R, tr = edit._similarity(None, ROTATION, TRANSLATION, 1.7)
    c = edit._Constants(s, R, tr, math.isqrt(K) - 1, single=True)
    model = 2 * 4 * (11 + 3 * K) * N
    out = {"N": N, "K": K, "model_bytes": model, "model_us_at_copy_rate": round(model / COPY_RATE * 1e6, 2)}
    got, want = edit._transform_hip(t, K, c), edit._transform_torch(t, K, c)
    out["bit_identical_to_the_definition"] = all(torch.equal(x.view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(got, want))
    del got, want
    outs = [torch.empty_like(x) for x in (t[0], t[1], t[2], t[4])]
    calls = {"transform_hip": lambda: edit._transform_hip(t, K, c),                  # outputs allocated inside, as a user's call
             "transform_hip_into": lambda: edit._transform_hip(t, K, c, out=outs),   # ... and into existing tensors: the launch alone
             "transform_torch": lambda: edit._transform_torch(t, K, c)}
    out.update(interleaved(calls, a.reps, a.iters, a.limit))
    h, tt = out["transform_hip"], out["transform_torch"]
    out["torch_over_hip"] = round(tt["median_ms"] / h["median_ms"], 2)
    out["hip_faster_by_more_than_the_spread"] = bool(tt["min_ms"] > h["max_ms"])
    out["hip_share_of_copy_rate"] = round(model / COPY_RATE * 1e3 / h["median_ms"], 3)
    out["hip_into_share_of_copy_rate"] = round(model / COPY_RATE * 1e3 / out["transform_hip_into"]["median_ms"], 3)
    return out


def psnr(a, b):
    mse = float((a.double() - b.double()).square().mean())
    return round(10.0 * math.log10(1.0 / mse), 2) if mse > 0 else float("inf")


def quality(dev):
    """A golden's scene (5000 Gaussians, 640 x 360, activated opacities) with degree-3 SH colours: its RGB as band 0, seeded
    higher bands; the frame of the transformed scene under the transformed camera against the frame of the scene itself."""
    sc, cam = randscene_v1(5000, 640, 360, ell=-3.0, seed=7, device=dev)
    g = torch.Generator().manual_seed(8)
    feats = torch.cat([((sc["features"] - 0.5) / SH_C0).unsqueeze(1), 0.15 * torch.randn((5000, 15, 3), generator=g).to(dev)], 1)
    sc = {**sc, "features": feats.contiguous()}

    def frame(d, camera):
        with torch.no_grad():
            return render_gaussians(d["means3d"], d["scales"], d["quats"], d["opacities"], d["features"], camera, sh_degree=3,
                                    backend="hip")

    ref = frame(sc, cam)
    out = {"scene": "randscene_v1(5000, 640, 360, ell=-3.0, seed=7), band 0 from its RGB, bands 1-3 0.15 randn (seed 8)",
           "frame_mean": round(float(ref.mean()), 4)}
    for s in (1.0, 2.0):
        kw = dict(rotation=ROTATION, translation=TRANSLATION, scale=s)
        out[f"psnr_s{s:g}_db"] = psnr(frame(transform_scene(sc, **kw), transform_camera(cam, **kw)), ref)
    # what leaving the SH coefficients alone costs (means, scales and quaternions moved, features kept)
    kw = dict(rotation=ROTATION, translation=TRANSLATION, scale=1.0)
    moved = transform_scene(sc, **kw)
    out["psnr_s1_coefficients_not_rotated_db"] = psnr(frame({**moved, "features": sc["features"]}, transform_camera(cam, **kw)), ref)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single timed step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transform_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transform_bench.py measures on a GPU: none is visible (no fallback)")
    dev = torch.device("cuda:0")
    _hip.lib()
    result = {"device": torch.cuda.get_device_name(dev), "rows_per_workgroup": {"K>1": _hip.TRANSFORM_ROWS, "K=1": _hip.TRANSFORM_ROWS_K1},
              "reps": a.reps, "calls_per_rep": a.iters,
              "what": "transform_hip: one launch of ms_scene_transform, outputs allocated inside; transform_hip_into: the same into "
                      "existing tensors; transform_torch: the torch definition of the same step on the same GPU; milliseconds per call "
                      "between two device events around calls_per_rep back-to-back calls, the variants alternating, after three "
                      "warm-up calls each; model: 4 (11 + 3 K) bytes read and written per Gaussian over 6.29 TB/s; quality: PSNR "
                      "(peak 1) of the frame of the transformed scene under the transformed camera against the frame of the scene "
                      "itself, recorded, not asserted"}
    for key, K in (("k1", 1), ("k16", 16)):
        result[key] = bench(a.n, K, dev, a)
        print(json.dumps({key: result[key]}), flush=True)
        torch.cuda.empty_cache()
    result["quality"] = quality(dev)
    print(json.dumps({"quality": result["quality"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
