"""What a frame costs when bins of the fused kernel run out of sorted front with pixels alive: finished in the kernel against
the clean-up launch kept (MOJOSPLAT_FUSED_SORT bit 2).  Per-frame wall times, synchronised.

  swap   config 3 on 32-px bins, frames 6 .. 9 render the same Gaussians with the near half nearly transparent (the scene swap
         of scripts/cut_miss_cost.py): the first of them is the frame whose bins continue at the default front level -- the
         lane then asks for deeper fronts / full sorts, which keep the two launches
  stack  4000 faint Gaussians over 64x64 (tests/test_hip_fused_cleanup.py, case 1), the lane put back on the default level
         after every frame: all four bins walk their whole lists every frame

python scripts/cleanup_in_kernel_cost.py [modes, e.g. 1,5 -- swap; stack runs them with the fused path forced]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import mojosplat_amd as ms
from mojosplat_amd import _fused, _hip
from mojosplat_amd.scenes import BACKGROUND_V1, randscene_v1
from mojosplat_amd.utils import Camera
from bench import WORKLOADS

modes = [int(m) for m in (sys.argv[1] if len(sys.argv) > 1 else "1,5").split(",")]
dev = torch.device("cuda:0")
g = lambda s: (s["means3d"], s["scales"], s["quats"], s["opacities"], s["features"])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 3)


N, W, H, ell, _ = WORKLOADS["cfg3"]
sc, cam = randscene_v1(N, W, H, ell=ell, device=dev)
other = dict(sc)
depth = (sc["means3d"] @ cam.R.T + cam.T)[:, 2]
other["opacities"] = torch.where(depth < depth.median(), sc["opacities"] * 0.02, sc["opacities"])
for mode in modes:
    _hip.config_fused_sort(mode)
    _fused._state.clear()
    _fused.FRAME_STATS = {}
    times, flags = [], []
    for k in range(14):
        s = sc if k < 6 or k >= 10 else other
        times.append(timed(lambda: ms.render_gaussians(*g(s), cam, backend="hip", bin_size=32)))
        flags.append(int(_fused._dev_state(dev, 0)["host_np"][7]) >> 48)
    print(json.dumps({"case": "swap cfg3", "fused_sort_mode": mode, "ms_per_frame_synchronised": times, "flag_bits_48_49": flags,
                      "swap_at_frames": [6, 10], "stats": _fused.FRAME_STATS}))
    _fused.FRAME_STATS = None

gen = torch.Generator().manual_seed(0)
n = 4000
st = dict(means3d=torch.stack([torch.rand(n, generator=gen) * 0.6 - 0.3, torch.rand(n, generator=gen) * 0.6 - 0.3,
                               4.0 + 2.0 * torch.rand(n, generator=gen)], 1),
          scales=torch.full((n, 3), -0.7) + 0.1 * torch.randn(n, 3, generator=gen),
          quats=torch.nn.functional.normalize(torch.randn(n, 4, generator=gen), dim=1),
          opacities=0.005 * (0.8 + 0.4 * torch.rand(n, generator=gen)), features=torch.rand(n, 3, generator=gen))
st = {k: v.to(dev) for k, v in st.items()}
scam = Camera(R=torch.eye(3, device=dev), T=torch.zeros(3, device=dev), H=64, W=64, fx=60.0, fy=60.0, cx=32.0, cy=32.0)
bg = torch.tensor(BACKGROUND_V1, device=dev)
for mode in modes:
    _hip.config_fused_sort((mode & 4) | 2)
    _fused._state.clear()
    _fused.FRAME_STATS = {}
    times = []
    for k in range(60):
        times.append(timed(lambda: ms.render_gaussians(*g(st), scam, background_color=bg, backend="hip", bin_size=32)))
        lane = _fused._dev_state(dev, 0)
        lane["full_sort"] = False
        lane["front_level"] = 0
    print(json.dumps({"case": "stack 4000 on 64x64", "fused_sort_mode": (mode & 4) | 2, "ms_per_frame_median_of_last_50": statistics.median(times[10:]),
                      "min": min(times[10:]), "stats": _fused.FRAME_STATS}))
    _fused.FRAME_STATS = None
