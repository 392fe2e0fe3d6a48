"""The MCMC strategy on one GPU: each of its three calls (mojosplat_amd/mcmc.py) -- inject_noise, relocate_dead, grow --
with backend="hip" (csrc/mcmc.hip) against backend="torch" (the definition, on the same GPU), alternated inside one run,
on 1 M Gaussians with (a) RGB colours, 14 floats per Gaussian, and (b) SH degree 3, 59 floats.  5 % of the rows are dead;
grow adds 5 %.  relocate_dead and grow have a GaussianAdam attached whose moments are populated.  Writes
profiles/mcmc_bench.json.  Fails without a GPU.

    python scripts/mcmc_bench.py [--reps 7] [--iters 5] [--out profiles/mcmc_bench.json]

relocate_dead consumes its input (no row is dead afterwards) and grow hands the optimiser new tensors, so every timed call
of those two gets fresh copies of the parameters and moments and a fresh optimiser, made outside the timed window.
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
from mojosplat_amd import GaussianAdam, _hip, grow, inject_noise, relocate_dead  # noqa: E402

COPY_RATE = 6.29e12                    # bytes/s: the copy rate DESIGN.md measured
N = 1_000_000
DEAD = 0.05
LR = 1.6e-4


def scene(feature_shape, dev):
    g = torch.Generator().manual_seed(11)
    opa = 0.02 + 0.97 * torch.rand(N, generator=g)
    opa[torch.rand(N, generator=g) < DEAD] = 0.001
    p = {"means3d": torch.randn((N, 3), generator=g), "scales": -5.0 + torch.rand((N, 3), generator=g),
         "quats": torch.randn((N, 4), generator=g), "opacities": torch.log(opa / (1 - opa)),
         "features": torch.rand((N, *feature_shape), generator=g)}
    p = {k: v.to(dev) for k, v in p.items()}
    moments = {k: (torch.randn(v.shape, generator=g).to(dev) * 1e-3, torch.rand(v.shape, generator=g).to(dev) * 1e-6) for k, v in p.items()}
    draws = torch.rand(N, dtype=torch.float64, generator=g).to(dev)
    noise = torch.randn((N, 3), generator=g).to(dev)
    return p, moments, draws, noise


def fresh(p, moments):
    q = {k: v.clone() for k, v in p.items()}
    opt = GaussianAdam(q, lr=1e-3, backend="hip")
    for k, v in q.items():
        opt.state[v] = {"step": torch.tensor(2.0), "exp_avg": moments[k][0].clone(), "exp_avg_sq": moments[k][1].clone()}
    return q, opt


def timed(fn):
    """Seconds between a host clock read after a device synchronise and the synchronise after the call."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def calls(p, moments, draws, noise):
    n_new = int(1.05 * N) - N

    def noise_call(backend):
        return timed(lambda: inject_noise(p, LR, noise=noise, backend=backend))

    def relocate_call(backend):
        q, opt = fresh(p, moments)
        return timed(lambda: relocate_dead(q, opt, draws=draws, backend=backend))

    def grow_call(backend):
        q, opt = fresh(p, moments)
        return timed(lambda: grow(q, opt, cap_max=2 * N, draws=draws[:n_new], backend=backend))

    return {"inject_noise": noise_call, "relocate_dead": relocate_call, "grow": grow_call}


def algorithm_bytes(call, floats, n_draws):
    """What the algorithm has to move.  noise: the row of scales, quaternion, opacity and noise read, the mean read and
    written.  sample: the opacity read, weight, count and flag written; the weight and flag read and the scan written; per
    draw the uniform and ~20 probes of the search, the source and target written.  apply: opacity, scales and count read and
    the new values written per row; per draw the source and target read, the source row of every copied tensor read and the
    target row written, the moments of source and target zeroed, the source's new opacity and scales written.  grow: besides,
    every parameter and both moments copied into the longer tensors."""
    if call == "inject_noise":
        return N * (12 + 12 + 16 + 4 + 12 + 12)
    per_row = (4 + 8 + 4 + 1) + (8 + 1 + 8) + (4 + 12 + 4 + 16)
    per_draw = (8 + 20 * 8 + 8 + 8) + 16 + 4 * (floats - 4) + 4 * floats + 2 * 2 * 4 * floats + 16
    moved = N * per_row + n_draws * per_draw
    return moved + (2 * 3 * 4 * floats * N if call == "grow" else 0)


def bench(label, feature_shape, a, dev):
    p, moments, draws, noise = scene(feature_shape, dev)
    floats = sum(v.numel() for v in p.values()) // N
    out = {"floats_per_gaussian": floats}
    for name, call in calls(p, moments, draws, noise).items():
        times = {"hip": [], "torch": []}
        for b in times:                                 # warm-up of every shape the timed window uses
            for _ in range(3):
                call(b)
        for _ in range(a.reps):
            for b in times:
                times[b].append(statistics.median(call(b)[0] for _ in range(a.iters)) * 1e3)
        res = call("hip")[1]
        n_draws = 0 if res is None else int(res.n)
        nbytes = algorithm_bytes(name, floats, n_draws)
        o = {"draws": n_draws, "bytes_the_algorithm_moves": int(nbytes)}
        for b, v in times.items():
            o[b] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                    "reps": len(v), "calls_per_rep": a.iters}
        rate = nbytes / (o["hip"]["median_ms"] * 1e-3)
        o["hip"].update(achieved_bytes_per_s=round(rate, 1), share_of_copy_rate_6_29TBs=round(rate / COPY_RATE, 4),
                        bound_ms_at_copy_rate=round(nbytes / COPY_RATE * 1e3, 4))
        o["torch_over_hip"] = round(o["torch"]["median_ms"] / o["hip"]["median_ms"], 3)
        o["hip_faster_by_more_than_the_spread"] = bool(o["torch"]["min_ms"] > o["hip"]["max_ms"])
        out[name] = o
        print(json.dumps({label: {name: o}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcmc_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcmc_bench.py measures on a GPU: none is visible (no fallback)")
    dev = torch.device("cuda:0")
    _hip.lib()
    result = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "calls_per_rep": a.iters, "gaussians": N,
              "dead_fraction": DEAD, "opacity_space": "logit",
              "what": "one call of inject_noise, relocate_dead (5 % of the rows dead) and grow (5 % more rows) over the five "
                      "tensors of a scene; the last two with a GaussianAdam attached (parameters and both moments move); host "
                      "clock from a device synchronise to the synchronise after the call, allocations inside; each rep is the "
                      "median of calls_per_rep calls, backends alternated rep by rep after warm-up; bytes: what the algorithm "
                      "has to move (see the script), against the 6.29 TB/s copy rate"}
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
