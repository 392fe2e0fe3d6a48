"""The k-nearest-neighbour search on one GPU (mojosplat_amd/knn.py, k = 3): ms_knn (csrc/knn.hip) at N = 100 k and 1 M, on
points uniform in a cube and on the means of randscene_v1 (a normal cloud: the density falls by orders of magnitude from the
centre outwards), with the Morton order's computation timed apart from the search; and the definition, knn_torch, on the same
GPU at N = 100 k only (N^2 work: at 1 M it is not worth running).  Writes profiles/knn_bench.json.  Fails without a GPU.

    python scripts/knn_bench.py [--reps 7] [--iters 3] [--torch-reps 3] [--out profiles/knn_bench.json]

The search is compute-bound on box tests and candidate distances, not on memory traffic: no bandwidth figure is given.
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
from mojosplat_amd import _hip, knn  # noqa: E402
from mojosplat_amd.knn import _knn_hip, knn_torch  # noqa: E402
from mojosplat_amd.scene_order import morton_permutation  # noqa: E402
from mojosplat_amd.scenes import randscene_v1  # noqa: E402

K = 3
SIZES = (100_000, 1_000_000)
TORCH_N = 100_000


def clouds(N, dev):
    uniform = torch.rand((N, 3), generator=torch.Generator().manual_seed(1))
    scene, _ = randscene_v1(N, 64, 64, seed=2)
    return {"uniform": uniform.to(dev), "randscene_v1": scene["means3d"].contiguous().to(dev)}


def timed(fn):
    """Milliseconds between a host clock read after a device synchronise and the synchronise after the call."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def stats(v, iters):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v),
            "calls_per_rep": iters}


def bench(p, a, with_torch):
    N = p.shape[0]
    order_of = lambda: morton_permutation(p).to(torch.int32)
    order = order_of()
    calls = {"order": order_of,                                             # the Morton permutation: torch ops
             "search": lambda: _knn_hip(p, N, K, True, order=order),        # ms_knn with the order in hand (outputs and workspace allocated inside)
             "knn": lambda: knn(p, k=K)}                                    # the public call: finite check, order, search
    for fn in calls.values():
        for _ in range(3):
            fn()
    times = {name: [] for name in calls}
    for _ in range(a.reps):
        for name, fn in calls.items():
            times[name].append(statistics.median(timed(fn)[0] for _ in range(a.iters)))
    out = {name: stats(v, a.iters) for name, v in times.items()}
    out["search_ns_per_point"] = round(out["search"]["median_ms"] * 1e6 / N, 3)
    d_as_stored = timed(lambda: _knn_hip(p, N, K, True, order=None))        # (what the order buys: one call, after the warm-up above)
    out["search_in_stored_order_ms"] = round(d_as_stored[0], 4)
    if with_torch:
        knn_torch(p, K)
        v = [timed(lambda: knn_torch(p, K))[0] for _ in range(a.torch_reps)]
        out["torch"] = stats(v, 1)
        out["torch_over_hip"] = round(out["torch"]["median_ms"] / out["knn"]["median_ms"], 2)
        out["hip_faster_by_more_than_the_spread"] = bool(out["torch"]["min_ms"] > out["knn"]["max_ms"])
        want, got = knn_torch(p, K), knn(p, k=K)
        out["bit_identical_to_the_definition"] = bool(torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench.py measures on a GPU: none is visible (no fallback)")
    dev = torch.device("cuda:0")
    _hip.lib()
    result = {"device": torch.cuda.get_device_name(dev), "k": K, "block": _hip.KNN_BLOCK, "reps": a.reps, "calls_per_rep": a.iters,
              "what": "order: morton_permutation(points) as int32 (torch ops); search: ms_knn with that order in hand, outputs and "
                      "workspace allocated inside; knn: the public call (finite check with its host wait, order, search); torch: "
                      "knn_torch, the chunked definition, on the same GPU (N = 100 k only); host clock from a device synchronise to "
                      "the synchronise after the call; each rep is the median of calls_per_rep calls (torch: one call per rep) "
                      "after warm-up; search_in_stored_order_ms: one call of ms_knn with order = NULL on the same points"}
    for N in SIZES:
        for name, p in clouds(N, dev).items():
            key = f"{name}_{N}"
            result[key] = bench(p, a, N == TORCH_N)
            print(json.dumps({key: result[key]}), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
