"""The bit packing of the viewer formats on one GPU (mojosplat_amd/splatio.py): one call of each of the four entry points of
csrc/splatio.hip -- ms_splat_compress, ms_splat_decompress, ms_splat32_pack, ms_splat32_unpack -- against the torch definition
of the same step on the same GPU and the same prepared inputs, at 1 M Gaussians with K = 1 and K = 16 (SH degree 3); and,
for one seeded scene of mojosplat_amd/scenes.py at a golden's size (5000 Gaussians, 640 x 360), the PSNR of the frame rendered
from the compressed-then-decompressed scene, and from the .splat rows, against the original frame.  The PSNRs are recorded,
not asserted: nothing here has a reference value to hold them against.  Writes profiles/splatio_bench.json.  Fails without a GPU.

    python scripts/splatio_bench.py [--n 1000000] [--reps 7] [--iters 5] [--limit 120] [--out profiles/splatio_bench.json]

Byte model of compress (what the README quotes): 13 floats and 3 (K - 1) floats read, 16 bytes and 3 (K - 1) bytes written per
Gaussian, 72 bytes per 256 of them; decompress moves the same bytes the other way; a .splat row reads 56 bytes and writes 32.
The share of the copy rate is that over the measured 6.29 TB/s of a float4 copy.  The torch ops that prepare the kernels' inputs
(sigmoid, exp, the quaternion's norm, the permutation) are the same for both backends and are not timed.  Every timed step
runs under its own time limit (--limit seconds, checked between calls).
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
from mojosplat_amd import _hip, compress_scene, decompress_scene, render_gaussians, splatio  # noqa: E402
from mojosplat_amd.knn import SH_C0  # noqa: E402
from mojosplat_amd.scenes import randscene_v1  # noqa: E402

COPY_RATE = 6.29e12           # bytes/s, the measured float4 copy rate of the MI355X


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


def same(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.uint8) if x.dtype != torch.uint8 else x,
                                                        y.view(torch.uint8) if y.dtype != torch.uint8 else y) for x, y in zip(a, b))


def bench(N, K, dev, a):
    p = scene(N, K, dev)
    t = splatio._validate_params(p, "hip")[2]
    perm = torch.arange(N, device=dev)
    pos, rot, lsc, rgba, shr = splatio._prepare(t, K, perm, "logit")
    scale_lin = torch.exp(p["scales"]).contiguous()
    R = 3 * (K - 1)
    C = -(-N // splatio.CHUNK)
    chunks, vertices, sh = splatio._compress_hip(pos, rot, lsc, rgba, shr)
    rows = splatio._splat32_pack_hip(pos, scale_lin, rgba, rot)
    compress_bytes = N * (52 + 4 * R + 16 + R) + 72 * C
    splat_bytes = N * (56 + 32)
    out = {"N": N, "K": K, "compress_model_bytes": compress_bytes, "compress_model_us_at_copy_rate": round(compress_bytes / COPY_RATE * 1e6, 2),
           "splat32_model_bytes": splat_bytes, "splat32_model_us_at_copy_rate": round(splat_bytes / COPY_RATE * 1e6, 2)}
    out["bit_identical_to_the_definition"] = bool(
        same((chunks, vertices, sh), splatio._compress_torch(pos, rot, lsc, rgba, shr)) and
        same(splatio._decompress_hip(chunks, vertices, sh), splatio._decompress_torch(chunks, vertices, sh)) and
        same((rows,), (splatio._splat32_pack_torch(pos, scale_lin, rgba, rot),)) and
        same(splatio._splat32_unpack_hip(rows), splatio._splat32_unpack_torch(rows)))
    calls = {"compress_hip": lambda: splatio._compress_hip(pos, rot, lsc, rgba, shr),
             "compress_torch": lambda: splatio._compress_torch(pos, rot, lsc, rgba, shr),
             "decompress_hip": lambda: splatio._decompress_hip(chunks, vertices, sh),
             "decompress_torch": lambda: splatio._decompress_torch(chunks, vertices, sh),
             "splat32_pack_hip": lambda: splatio._splat32_pack_hip(pos, scale_lin, rgba, rot),
             "splat32_pack_torch": lambda: splatio._splat32_pack_torch(pos, scale_lin, rgba, rot),
             "splat32_unpack_hip": lambda: splatio._splat32_unpack_hip(rows),
             "splat32_unpack_torch": lambda: splatio._splat32_unpack_torch(rows)}
    out.update(interleaved(calls, a.reps, a.iters, a.limit))
    for d, model in (("compress", compress_bytes), ("decompress", compress_bytes), ("splat32_pack", splat_bytes), ("splat32_unpack", splat_bytes)):
        h, tt = out[d + "_hip"], out[d + "_torch"]
        out[d + "_torch_over_hip"] = round(tt["median_ms"] / h["median_ms"], 2)
        out[d + "_hip_faster_by_more_than_the_spread"] = bool(tt["min_ms"] > h["max_ms"])
        out[d + "_hip_share_of_copy_rate"] = round(model / COPY_RATE * 1e3 / h["median_ms"], 3)
    return out


def psnr(a, b):
    mse = float((a.double() - b.double()).square().mean())
    return round(10.0 * math.log10(1.0 / mse), 2) if mse > 0 else float("inf")


def quality(dev):
    """A golden's scene (5000 Gaussians, 640 x 360, activated opacities, RGB colours) through both formats and back."""
    sc, cam = randscene_v1(5000, 640, 360, ell=-3.0, seed=7, device=dev)

    def frame(d):
        colours = d["features"] if d["features"].dim() == 2 else (d["features"][:, 0] * SH_C0 + 0.5).contiguous()
        with torch.no_grad():
            return render_gaussians(d["means3d"], d["scales"], d["quats"], d["opacities"], colours, cam, backend="hip")

    ref = frame(sc)
    back = decompress_scene(compress_scene(sc, opacity_space="linear"), opacity_space="linear")
    rows, _ = splatio.pack_splat_rows(sc, opacity_space="linear")
    splat = splatio.unpack_splat_rows(rows, opacity_space="linear")
    return {"scene": "randscene_v1(5000, 640, 360, ell=-3.0, seed=7)", "psnr_compressed_ply_db": psnr(frame(back), ref),
            "psnr_splat_db": psnr(frame(splat), ref), "frame_mean": round(float(ref.mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single timed step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splatio_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("splatio_bench.py measures on a GPU: none is visible (no fallback)")
    dev = torch.device("cuda:0")
    _hip.lib()
    result = {"device": torch.cuda.get_device_name(dev), "rows_per_workgroup": _hip.SPLAT_CHUNK, "reps": a.reps, "calls_per_rep": a.iters,
              "what": "*_hip: one launch of the entry point on prepared inputs, outputs allocated inside; *_torch: the torch definition "
                      "of the same step on the same GPU; milliseconds per call between two device events around calls_per_rep "
                      "back-to-back calls, the eight variants alternating, after three warm-up calls each; model: the bytes each "
                      "array is read or written once over 6.29 TB/s; quality: PSNR (peak 1) of the frame rendered from the scene after "
                      "compress + decompress, and after the .splat rows, against the frame of the scene itself, recorded, not asserted"}
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
