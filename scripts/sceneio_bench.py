"""The row move of scene files on one GPU (mojosplat_amd/sceneio.py): pack_ply_rows and unpack_ply_rows with backend="hip"
(ms_ply_pack / ms_ply_unpack, csrc/sceneio.hip) against backend="torch" (the definition: int32 views moved by torch indexing) on
the same GPU and the same data, at 1 M Gaussians with (N, 3) RGB features (a row of 17 floats) and with SH degree 3 (62
floats); and, apart from those, whole save_ply / load_ply calls to a temporary file (disk and host copies included: not the
kernel's time).  Writes profiles/sceneio_bench.json.  Fails without a GPU.

    python scripts/sceneio_bench.py [--n 1000000] [--reps 7] [--iters 5] [--file-reps 3] [--limit 120] [--out profiles/sceneio_bench.json]

Byte model of the row move: every float of a row is read once and written once, 2 * 4 F bytes per Gaussian (the three
columns of zeros are written and not read: 12 bytes per row fewer); the share of the copy rate is that over the measured
6.29 TB/s of a float4 copy.  Every timed step runs under its own time limit (--limit seconds, checked between calls).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from mojosplat_amd import _hip, load_ply, pack_ply_rows, save_ply, unpack_ply_rows  # noqa: E402
from mojosplat_amd.sceneio import property_names  # noqa: E402

COPY_RATE = 6.29e12           # bytes/s, the measured float4 copy rate of the MI355X


class StepTimeout(RuntimeError):
    pass


def scene(N, K, dev, rgb):
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(s, generator=g).to(dev)
    return {"means3d": r(N, 3), "scales": r(N, 3) - 4.0, "quats": r(N, 4), "opacities": r(N),
            "features": torch.rand((N, 3), generator=g).to(dev) if rgb else r(N, K, 3)}


def timed_events(fn, iters):
    """Milliseconds per call between two device events around `iters` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def timed_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}


def interleaved(calls, reps, timer, limit):
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
            times[name].append(timer(fn))
            if time.perf_counter() - t0 > limit:
                raise StepTimeout(f"{name}: one timed step took more than {limit} s")
    return {name: stats(v) for name, v in times.items()}


def bench(N, K, rgb, dev, a):
    p = scene(N, K, dev, rgb)
    K = 1 if rgb else K
    F = 14 + 3 * K
    names = property_names(K)
    rows = pack_ply_rows(p)
    sh = {**p, "features": unpack_ply_rows(rows, names)["features"]}     # (SH features: the move alone, no conversion)
    out = {"N": N, "K": K, "F": F, "rgb_input": rgb, "model_bytes": 2 * 4 * F * N,
           "model_us_at_copy_rate": round(2 * 4 * F * N / COPY_RATE * 1e6, 2)}
    out["bit_identical_to_the_definition"] = bool(
        torch.equal(rows.view(torch.int32), pack_ply_rows(p, backend="torch").view(torch.int32)) and
        all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in
            zip(unpack_ply_rows(rows, names).values(), unpack_ply_rows(rows, names, backend="torch").values())))
    calls = {"pack_hip": lambda: pack_ply_rows(sh), "pack_torch": lambda: pack_ply_rows(sh, backend="torch"),
             "unpack_hip": lambda: unpack_ply_rows(rows, names), "unpack_torch": lambda: unpack_ply_rows(rows, names, backend="torch")}
    out.update(interleaved(calls, a.reps, lambda fn: timed_events(fn, a.iters), a.limit))
    for d in ("pack", "unpack"):
        h, t = out[d + "_hip"], out[d + "_torch"]
        out[d + "_torch_over_hip"] = round(t["median_ms"] / h["median_ms"], 2)
        out[d + "_hip_faster_by_more_than_the_spread"] = bool(t["min_ms"] > h["max_ms"])
        out[d + "_hip_share_of_copy_rate"] = round(out["model_us_at_copy_rate"] * 1e-3 / h["median_ms"], 3)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scene.ply")
        files = {"save_hip": lambda: save_ply(path, p), "load_hip": lambda: load_ply(path),
                 "save_torch": lambda: save_ply(path, p, backend="torch"), "load_torch": lambda: load_ply(path, backend="torch", device=dev)}
        out["files"] = interleaved(files, a.file_reps, timed_host, a.limit)
        out["files"]["bytes"] = os.path.getsize(path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--file-reps", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single timed step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sceneio_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sceneio_bench.py measures on a GPU: none is visible (no fallback)")
    dev = torch.device("cuda:0")
    _hip.lib()
    result = {"device": torch.cuda.get_device_name(dev), "rows_per_workgroup": _hip.PLY_ROWS, "reps": a.reps, "calls_per_rep": a.iters,
              "what": "pack_* / unpack_*: pack_ply_rows / unpack_ply_rows on SH features (no conversion), outputs allocated inside; "
                      "milliseconds per call between two device events around calls_per_rep back-to-back calls, the four variants "
                      "alternating, after three warm-up calls each; model: 2 * 4 F bytes per Gaussian over 6.29 TB/s; files: whole "
                      "save_ply / load_ply calls to a temporary file, host clock from a device synchronise to the synchronise "
                      "after the call (disk, page cache and host copies included); *_torch: backend='torch' on the same GPU"}
    for key, K, rgb in (("rgb", 1, True), ("sh3", 16, False)):
        result[key] = bench(a.n, K, rgb, dev, a)
        print(json.dumps({key: result[key]}), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
