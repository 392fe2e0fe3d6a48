"""SH backward with and without the camera-centre gradient (k_sh_bwd<3, false | true> + k_pose_slab_sum<3>), for
rocprofv3 --kernel-trace --stats:  python scripts/sh_pose_probe.py [N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mojosplat_amd.scenes import randscene_v1
from mojosplat_amd.sh import evaluate_sh_hip

dev = torch.device("cuda:0")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
sc, cam = randscene_v1(N, 1920, 1080, ell=-4.0, seed=42, device=dev)
coeffs = (torch.randn(N, 16, 3, generator=torch.Generator().manual_seed(1)) * 0.3).to(dev).requires_grad_(True)
means = sc["means3d"].clone().requires_grad_(True)
v = torch.rand(N, 3, device=dev)
for pose in (False, True):
    vm = cam.view_matrix.detach().clone().requires_grad_(pose)
    c = type(cam)(R=cam.R, T=cam.T, H=cam.H, W=cam.W, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, view_matrix=vm)
    for _ in range(25):
        evaluate_sh_hip(means, coeffs, c, 3).backward(v)
    torch.cuda.synchronize()
    print("pose" if pose else "no pose", "v_viewmat" if pose else "", vm.grad.flatten()[:4].tolist() if pose else "")
