"""The densification step of 3DGS training on one GPU: one densify_and_prune call (mojosplat_amd/refine.py) -- its single
host wait included -- with a GaussianAdam attached whose moments are populated, backend="hip" (csrc/densify.hip) against
backend="torch" (the definition, on the same GPU), alternated inside one run, on 1 M Gaussians with (a) RGB colours, 14
floats per Gaussian, and (b) SH degree 3, 59 floats.  Statistics and scales are synthesised so that roughly 5 % of the rows
are cloned, 5 % split and 5 % pruned.  Writes profiles/densify_bench.json.  Fails without a GPU.

    python scripts/densify_bench.py [--reps 7] [--iters 5] [--out profiles/densify_bench.json]

A call consumes its inputs (the optimiser adopts the new tensors), so every timed call gets a fresh optimiser over the same
parameter tensors and moments; building it is host work of a few microseconds outside the timed window.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from mojosplat_amd import DensifyStats, GaussianAdam, _hip, densify_and_prune  # noqa: E402

COPY_RATE = 6.29e12                    # bytes/s: the copy rate DESIGN.md measured
N = 1_000_000
RULES = dict(grow_grad2d=2e-4, grow_scale3d=0.01, grow_scale2d=0.05, prune_opa=0.005, prune_scale3d=0.1, prune_scale2d=0.15,
             scene_scale=1.0)


def scene(feature_shape, dev):
    """Parameters, moments and statistics: 10 % of the rows have a high gradient, half of them small (clone) and half large
    (split); 5 % are transparent (pruned).  Nothing is wide on screen or too big."""
    g = torch.Generator().manual_seed(11)
    r = torch.rand(N, generator=g)
    high, small, faint = r < 0.105, torch.rand(N, generator=g) < 0.5, torch.rand(N, generator=g) < 0.05
    smax = torch.where(high & ~small, -3.5 - torch.rand(N, generator=g), -5.0 - torch.rand(N, generator=g))
    p = {"means3d": torch.randn((N, 3), generator=g), "scales": smax[:, None] - torch.rand((N, 3), generator=g),
         "quats": torch.randn((N, 4), generator=g), "opacities": torch.where(faint, 0.001, 0.1 + 0.8 * torch.rand(N, generator=g)),
         "features": torch.rand((N, *feature_shape), generator=g)}
    p["scales"][:, 0] = smax
    stats = DensifyStats(N, dev)
    stats.count.fill_(4.0)
    stats.grad2d.copy_(torch.where(high, 4e-4, 1e-4) * 4.0)
    stats.max_radii.fill_(0.01)
    p = {k: v.to(dev) for k, v in p.items()}
    moments = {k: (torch.randn(v.shape, generator=g).to(dev) * 1e-3, torch.rand(v.shape, generator=g).to(dev) * 1e-6) for k, v in p.items()}
    noise = torch.randn((2, N, 3), generator=g).to(dev)
    return p, moments, stats, noise


def one_call(p, moments, stats, noise, backend):
    """(seconds of one call between a host clock read after a device synchronise and the call's return + a synchronise)."""
    opt = GaussianAdam(p, lr=1e-3, backend="hip")
    for k, v in p.items():
        opt.state[v] = {"step": torch.tensor(2.0), "exp_avg": moments[k][0], "exp_avg_sq": moments[k][1]}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = densify_and_prune(p, stats, opt, noise=noise, backend=backend, **RULES)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def bench(label, feature_shape, a, dev):
    p, moments, stats, noise = scene(feature_shape, dev)
    floats = sum(v.numel() for v in p.values()) // N
    times = {"hip": [], "torch": []}
    for b in times:                                     # warm-up of every shape the timed window uses
        for _ in range(3):
            _, res = one_call(p, moments, stats, noise, b)
    for _ in range(a.reps):
        for b in times:
            times[b].append(statistics.median(one_call(p, moments, stats, noise, b)[0] for _ in range(a.iters)) * 1e3)
    _, hip = one_call(p, moments, stats, noise, "hip")
    _, ref = one_call(p, moments, stats, noise, "torch")
    same = torch.equal(hip.source, ref.source) and all(
        torch.equal(hip.params[k] if k != "means3d" else hip.params[k][:hip.n_kept + hip.n_cloned],
                    ref.params[k] if k != "means3d" else ref.params[k][:ref.n_kept + ref.n_cloned]) for k in p)
    n_out = hip.source.numel()
    # what the algorithm has to move: classify reads 28 bytes and writes a flag byte per row; the move reads the flag and
    # every source row that leaves an output (parameter + two moments), reads the noise of split rows, and writes every
    # output row (parameter + two moments) and its source index
    surviving = N - hip.n_pruned
    nbytes = N * 29 + N * 1 + surviving * 12 * floats + hip.n_split * 24 + n_out * (12 * floats + 8)
    out = {"floats_per_gaussian": floats, "rows_in": N, "rows_out": n_out, "kept": hip.n_kept, "cloned": hip.n_cloned,
           "split": hip.n_split, "pruned": hip.n_pruned, "outputs_equal_to_the_definition_on_the_same_gpu": bool(same),
           "bytes_the_algorithm_moves": int(nbytes)}
    for b, v in times.items():
        med = statistics.median(v)
        out[b] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v),
                  "calls_per_rep": a.iters}
    rate = nbytes / (out["hip"]["median_ms"] * 1e-3)
    out["hip"].update(achieved_bytes_per_s=round(rate, 1), share_of_copy_rate_6_29TBs=round(rate / COPY_RATE, 4),
                      bound_ms_at_copy_rate=round(nbytes / COPY_RATE * 1e3, 4))
    out["torch_over_hip"] = round(out["torch"]["median_ms"] / out["hip"]["median_ms"], 3)
    out["hip_faster_by_more_than_the_spread"] = bool(out["torch"]["min_ms"] > out["hip"]["max_ms"])
    print(json.dumps({label: out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("densify_bench.py measures on a GPU: none is visible (no fallback)")
    dev = torch.device("cuda:0")
    _hip.lib()
    result = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "calls_per_rep": a.iters, "gaussians": N,
              "what": "one densify_and_prune call over the five tensors of a scene with a GaussianAdam attached (parameters and "
                      "both moments move), host clock from a device synchronise to the synchronise after the call: its one "
                      "host wait, its allocations and the zeroed statistics are inside; each rep is the median of "
                      "calls_per_rep calls, backends alternated rep by rep after warm-up; bytes: what the algorithm has to "
                      "move (see the script), against the 6.29 TB/s copy rate"}
    result["rgb"] = bench("rgb", (3,), a, dev)
    torch.cuda.empty_cache()
    result["sh3"] = bench("sh3", (16, 3), a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
