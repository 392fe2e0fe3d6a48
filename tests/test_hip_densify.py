"""GPU: the densification statistics that render_gaussians_trainable(..., densify=DensifyStats) accumulates in its
backward (densify.py; include/mojosplat_hip.h, ms_render_bwd_finish_densify / ms_densify_stats_update).

The definition is densify.update_torch fed with the view's dL/dmeans2d and the forward projection's radii.  count and
max_radii depend on the geometry only and are compared exactly; grad2d with the gradient bars of test_hip_backward.py
(float64 autograd of the restatement; fused against per-stage: two fp32 implementations)."""
import ctypes
import math
import os

import pytest
import torch

from helpers import assert_grad_close, simple_camera
from mojosplat_amd import _hip
from mojosplat_amd.autograd import project_gaussians_autograd, rasterize_gaussians_autograd, render_gaussians_trainable
from mojosplat_amd.binning import bin_gaussians_to_tiles_hip
from mojosplat_amd.densify import DensifyStats, update_torch
from mojosplat_amd.projection import EPS2D, project_gaussians_hip
from mojosplat_amd.scenes import randscene_v1
from mojosplat_amd.utils import Camera, look_at
from oracle import torch_oracle

pytestmark = pytest.mark.gpu

NAMES = ("means3d", "scales", "quats", "opacities", "features")
ELEM_F64 = 2e-3                                 # as test_hip_backward.py
FUSED = dict(elem_rel=5e-3, elem_p999=1e-3)     # as test_hip_backward.py
# grad2d against float64 autograd: the max-norm bar of test_end_to_end_gradients_and_finite_difference (5e-3) and its
# per-element bar on the 99.9th percentile; the worst element gets 10x.  The fused frame's screen gradient is
# (a gx + b gy, b gx + c gy) of raw sums over the footprint (rasterize_bwdq.hip), which cancel for a Gaussian whose
# pixels pull every way: a small |dL/dmeans2d| keeps fewer relative digits than the 3D gradients it feeds (measured
# at 12k Gaussians, 640x480: worst 8.3e-3, 99.9th percentile 2.2e-4).
F64_2D = dict(rel=5e-3, elem_rel=10 * ELEM_F64, elem_p999=ELEM_F64)


def _cam_args(cam):
    return (cam.view_matrix.double().cpu(), cam.fx, cam.fy, cam.cx, cam.cy, cam.W, cam.H)


def _v_img(H, W, C=3, seed=5):
    return torch.rand(H, W, C, generator=torch.Generator().manual_seed(seed))


def _train(sc, cam, bg, v_img, **kw):
    """One view through render_gaussians_trainable with fresh statistics -> (stats, image, leaves)."""
    dev = sc["means3d"].device
    st = kw.pop("stats", None) or DensifyStats(sc["means3d"].shape[0], dev)
    leaves = [sc[k].clone().requires_grad_(True) for k in NAMES]
    img = render_gaussians_trainable(*leaves, cam, background_color=bg, densify=st, **kw)
    (img * v_img.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return st, img.detach(), leaves


def _per_stage_reference(sc, cam, bg, v_img, tile_size=16, features=None):
    """update_torch fed with the per-stage functions' own means2d gradient (retain_grad) and radii."""
    dev = sc["means3d"].device
    leaves = [sc[k].clone().requires_grad_(True) for k in NAMES[:4]]
    feats = sc["features"] if features is None else features
    m2, con, dep, rad = project_gaussians_autograd(*leaves, cam)
    m2.retain_grad()
    th, tw = -(-cam.H // tile_size), -(-cam.W // tile_size)
    with torch.no_grad():
        ids, ranges = bin_gaussians_to_tiles_hip(m2, rad, dep, tile_size, tw, th)
    img = rasterize_gaussians_autograd(m2, con, feats, leaves[3], bg, ranges, ids, cam, tile_size)
    (img * v_img.to(dev)).sum().backward()
    return update_torch(DensifyStats(m2.shape[0], "cpu"), m2.grad.cpu(), rad.cpu(), cam.W, cam.H), rad


def _assert_stats(tag, got, ref, **bars):
    assert torch.equal(got.count.cpu(), ref.count.cpu()), f"{tag}: count"
    assert torch.equal(got.max_radii.cpu(), ref.max_radii.cpu()), f"{tag}: max_radii"
    assert_grad_close(f"{tag}/grad2d", got.grad2d.cpu(), ref.grad2d.cpu(), **bars)


@pytest.mark.parametrize("N,W,H,ell", [(2000, 256, 256, -3.0), (12000, 640, 480, -3.5)])
def test_fused_frame_statistics_vs_float64_autograd(device, N, W, H, ell):
    sc, cam = randscene_v1(N, W, H, ell=ell, seed=31, device=device)
    bg = torch.tensor([0.1, 0.2, 0.3], device=device)
    v_img = _v_img(H, W)
    st, img, leaves = _train(sc, cam, bg, v_img)
    with torch.no_grad():
        m2h, conh, deph, radh = project_gaussians_hip(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], cam)
    alive = (radh > 0).all(-1)
    assert 0 < int(alive.sum()) < N and int(st.count.sum()) == int(alive.sum())
    ids, ranges = bin_gaussians_to_tiles_hip(m2h, radh, deph, 16, -(-W // 16), -(-H // 16))
    rl = [sc[k].detach().double().cpu().requires_grad_(True) for k in NAMES]
    rm2, rcon, _ = torch_oracle.project(rl[0], rl[1], rl[2], *_cam_args(cam))
    rm2.retain_grad()
    rimg, _ = torch_oracle.rasterize(rm2, rcon, rl[4], rl[3], bg.double().cpu(), ranges.cpu(), ids.cpu(), H, W, 16)
    (rimg * v_img.double()).sum().backward()
    ref = update_torch(DensifyStats(N, "cpu"), rm2.grad, radh.cpu(), W, H)
    _assert_stats(f"f64 {N}", st, ref, **F64_2D)
    assert (st.grad2d[~alive] == 0).all() and (st.grad2d > 0).any()


def test_fused_frame_statistics_at_config3_size_vs_per_stage(device):
    N, W, H = 1_000_000, 1920, 1080
    sc, cam = randscene_v1(N, W, H, ell=-4.0, seed=42, device=device)
    bg = torch.tensor([0.1, 0.1, 0.1], device=device)
    v_img = _v_img(H, W)
    fused, img_f, _ = _train(sc, cam, bg, v_img)
    stage, img_s, _ = _train(sc, cam, bg, v_img, stagewise=True)
    assert torch.equal(img_f, img_s)
    assert int(fused.count.sum()) > N // 10
    _assert_stats("cfg3", fused, stage, rel=1e-4, **FUSED)


def test_orbiting_views_accumulate(device):
    N, W, H = 6000, 320, 240
    sc, cam0 = randscene_v1(N, W, H, ell=-3.5, seed=7, device=device)
    bg = torch.tensor([0.0, 0.0, 0.0], device=device)
    cams = []
    for k in range(4):
        a = 2 * math.pi * k / 4 + 0.3
        vm = look_at(torch.tensor([5.0 * math.sin(a), 1.5, 5.0 * math.cos(a)]), torch.zeros(3), torch.tensor([0.0, 1.0, 0.0]))
        cams.append(Camera(R=vm[:3, :3].contiguous().to(device), T=vm[:3, 3].contiguous().to(device), H=H, W=W,
                           fx=cam0.fx, fy=cam0.fy, cx=cam0.cx, cy=cam0.cy, near=cam0.near, far=cam0.far))
    acc = DensifyStats(N, device)
    singles = []
    for k, cam in enumerate(cams):
        _train(sc, cam, bg, _v_img(H, W, seed=k), stats=acc)
        singles.append(_train(sc, cam, bg, _v_img(H, W, seed=k))[0])
    ref = DensifyStats(N, device)
    for s in singles:
        ref.grad2d += s.grad2d
        ref.count += s.count
        ref.max_radii = torch.maximum(ref.max_radii, s.max_radii)
    assert int(acc.count.max()) >= 2
    _assert_stats("orbit", acc, ref, rel=1e-4, **FUSED)


def _edge_scene(device):
    """simple_camera (64x64, f = 100, looking down +z).  0-2: three near-opaque wide layers at z = 2 (T < 1e-4 behind
    their centre); 3: a small Gaussian fully hidden behind them; 4: behind the near plane; 5: off-screen; 6: opacity
    below 1/255; 7: a small one in front of everything."""
    m = [[0, 0, 2.0], [0.01, 0, 2.01], [0, 0.01, 2.02], [0, 0, 5.0], [0.1, 0, 0.05], [6.0, 0, 3.0], [0.2, 0.1, 1.5],
         [0.3, 0.3, 1.5]]
    s = [0.0, 0.0, 0.0, math.log(0.03), math.log(0.05), math.log(0.05), math.log(0.05), math.log(0.05)]
    op = [0.9999, 0.9999, 0.9999, 0.9, 0.9, 0.9, 0.003, 0.8]
    n = len(m)
    sc = dict(means3d=torch.tensor(m), scales=torch.tensor(s)[:, None].repeat(1, 3),
              quats=torch.tensor([[1.0, 0, 0, 0]]).repeat(n, 1), opacities=torch.tensor(op),
              features=torch.rand(n, 3, generator=torch.Generator().manual_seed(1)))
    return {k: v.float().contiguous().to(device) for k, v in sc.items()}, simple_camera(device)


@pytest.mark.parametrize("stagewise", [False, True])
def test_culled_and_hidden_gaussians(device, stagewise):
    sc, cam = _edge_scene(device)
    bg = torch.tensor([0.5, 0.5, 0.5], device=device)
    st = DensifyStats(8, device)
    st.grad2d.fill_(0.5), st.count.fill_(2.0), st.max_radii.fill_(0.25)
    _, _, leaves = _train(sc, cam, bg, _v_img(64, 64), stats=st, stagewise=stagewise)
    rad = project_gaussians_hip(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], cam)[3]
    assert (rad[[0, 1, 2, 3, 7]] > 0).all() and (rad[[4, 5, 6]] == 0).all()
    assert (leaves[0].grad[3] == 0).all() and (leaves[3].grad[3] == 0)    # the hidden one was never blended ...
    assert st.count.tolist() == [3.0, 3.0, 3.0, 3.0, 2.0, 2.0, 2.0, 3.0]  # ... and still counts
    g = st.grad2d.tolist()
    assert g[3] == 0.5 and g[4] == g[5] == g[6] == 0.5 and g[7] > 0.5 and g[0] > 0.5
    assert st.max_radii[[4, 5, 6]].tolist() == [0.25] * 3
    assert st.max_radii[0].item() == max(0.25, rad[0].max().item() / 64)


def _hip_memcpy_d2d(dst_ptr, src_ptr, nbytes, stream):
    for name in ("libamdhip64.so", os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")):
        try:
            hip = ctypes.CDLL(name)
            break
        except OSError:
            continue
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    assert hip.hipMemcpyAsync(dst_ptr, src_ptr, nbytes, 3, stream) == 0   # hipMemcpyDeviceToDevice


def test_finish_with_statistics_writes_bit_identical_gradients(device, monkeypatch):
    """ms_render_bwd_finish and ms_render_bwd_finish_densify on the same rows (a real frame's, then with some zeroed)."""
    N, W, H = 20000, 640, 480
    sc, cam = randscene_v1(N, W, H, ell=-3.5, seed=3, device=device)
    bg = torch.tensor([0.1, 0.1, 0.1], device=device)
    L = _hip.lib()
    rows = torch.zeros(N * 16, dtype=torch.float32, device=device)
    finish = L.ms_render_bwd_finish

    def capture(*args):   # the frame's own finish, and a copy of the rows it finishes
        _hip_memcpy_d2d(ctypes.c_void_p(rows.data_ptr()), args[15], N * 64, args[-1])
        return finish(*args)
    monkeypatch.setattr(L, "ms_render_bwd_finish", capture)
    leaves = [sc[k].clone().requires_grad_(True) for k in NAMES]
    (render_gaussians_trainable(*leaves, cam, background_color=bg) * _v_img(H, W).to(device)).sum().backward()
    monkeypatch.undo()
    torch.cuda.synchronize()
    R = rows.view(N, 16)
    assert (R[:, :6] != 0).any(-1).sum() > N // 10

    vm = cam._viewmat_f32().to(device)
    m3, s3, q4, op = (sc[k].contiguous() for k in NAMES[:4])
    for zero_every in (None, 3):
        if zero_every:
            R[::zero_every] = 0
        outs = []
        for with_stats in (False, True):
            o = [torch.full((N, k), float("nan"), device=device) for k in (3, 3, 4, 1, 3)]
            common = (N, _hip.ptr(m3), _hip.ptr(s3), 1, _hip.ptr(q4), _hip.ptr(op), 3, _hip.ptr(vm), cam.fx, cam.fy, cam.cx,
                      cam.cy, W, H, EPS2D, _hip.ptr(rows)) + tuple(_hip.ptr(t) for t in o)
            if with_stats:
                st = DensifyStats(N, device)
                _hip.check(L.ms_render_bwd_finish_densify(*common, cam.near, cam.far, _hip.ptr(st.grad2d), _hip.ptr(st.count),
                                                          _hip.ptr(st.max_radii), _hip.stream(device)))
            else:
                _hip.check(L.ms_render_bwd_finish(*common, _hip.stream(device)))
            torch.cuda.synchronize()
            outs.append(o)
        for a, b in zip(*outs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        rad = project_gaussians_hip(m3, s3, q4, op, cam)[3]
        alive = (rad > 0).all(-1)
        assert torch.equal(st.count, alive.float())
        blended = (R[:, :6] != 0).any(-1)
        assert (st.grad2d[~blended] == 0).all() and (st.grad2d[blended & alive] > 0).any()


def test_statistics_do_not_disturb_the_frame(device):
    """Same image bit for bit; gradients within the run-to-run noise of the backward rasteriser's row atomics (the bars
    of two fp32 runs: the ABI test above shows the finish itself writes the same bits)."""
    N, W, H = 20000, 640, 480
    sc, cam = randscene_v1(N, W, H, ell=-3.5, seed=9, device=device)
    bg = torch.tensor([0.2, 0.1, 0.3], device=device)
    v_img = _v_img(H, W)
    st, img1, l1 = _train(sc, cam, bg, v_img)
    leaves = [sc[k].clone().requires_grad_(True) for k in NAMES]
    img0 = render_gaussians_trainable(*leaves, cam, background_color=bg)
    (img0 * v_img.to(device)).sum().backward()
    assert torch.equal(img0.detach(), img1)
    for name, a, b in zip(NAMES, leaves, l1):
        assert_grad_close(f"undisturbed/{name}", a.grad, b.grad, rel=1e-4, **FUSED)


VARIANTS = {
    "C1": dict(channels=1),
    "C4": dict(channels=4),
    "fp16": dict(fp16=True),
    "ts8": dict(tile_size=8),
    "ts24": dict(tile_size=24),
    "stagewise": dict(stagewise=True),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_per_stage_route_matches_the_fused_one(device, variant):
    """Any frame that is not lean takes the per-stage route for its statistics: the same count / max_radii as the
    lean fused frame of the same geometry, and grad2d equal to update_torch of the per-stage functions' own means2d
    gradient (three-channel routes also against the fused frame's grad2d)."""
    kw = dict(VARIANTS[variant])
    N, W, H = 8000, 400, 304
    C = kw.pop("channels", 3)
    fp16 = kw.pop("fp16", False)
    sc, cam = randscene_v1(N, W, H, ell=-3.5, seed=23, device=device, channels=C)
    sc3, _ = randscene_v1(N, W, H, ell=-3.5, seed=23, device=device)
    if fp16:
        sc["features"] = sc["features"].half()
    bg = torch.full((C,), 0.1, device=device)
    v_img = _v_img(H, W, C)
    fused, _, _ = _train(sc3, cam, torch.full((3,), 0.1, device=device), _v_img(H, W, 3))
    st, _, _ = _train(sc, cam, bg, v_img, **kw)
    ref, rad = _per_stage_reference(sc, cam, bg, v_img, tile_size=kw.get("tile_size", 16))
    assert torch.equal(st.count, fused.count) and torch.equal(st.max_radii, fused.max_radii)
    _assert_stats(variant, st, ref, rel=1e-4, **FUSED)
    if C == 3 and not fp16:
        assert_grad_close(f"{variant}/vs-fused", st.grad2d, fused.grad2d, rel=1e-4, **FUSED)


def test_sh_features_fused_and_per_stage(device):
    N, W, H, deg = 6000, 320, 240, 2
    sc, cam = randscene_v1(N, W, H, ell=-3.5, seed=29, device=device)
    K = (deg + 1) ** 2
    sc["features"] = (torch.randn(N, K, 3, generator=torch.Generator().manual_seed(2)) * 0.3).to(device)
    bg = torch.tensor([0.1, 0.1, 0.1], device=device)
    v_img = _v_img(H, W)
    fused, img_f, _ = _train(sc, cam, bg, v_img, sh_degree=deg)
    stage, img_s, _ = _train(sc, cam, bg, v_img, sh_degree=deg, stagewise=True)
    assert torch.equal(img_f, img_s) and int(fused.count.sum()) > 0
    _assert_stats("sh", fused, stage, rel=1e-4, **FUSED)


@pytest.mark.parametrize("stagewise", [False, True])
def test_second_backward_does_not_update_again(device, stagewise):
    N, W, H = 4000, 256, 256
    sc, cam = randscene_v1(N, W, H, ell=-3.0, seed=13, device=device)
    st = DensifyStats(N, device)
    leaves = [sc[k].clone().requires_grad_(True) for k in NAMES]
    img = render_gaussians_trainable(*leaves, cam, densify=st, stagewise=stagewise)
    loss = (img * _v_img(H, W).to(device)).sum()
    loss.backward(retain_graph=True)
    once = [t.clone() for t in (st.grad2d, st.count, st.max_radii)]
    assert once[1].sum() > 0
    loss.backward()
    assert all(torch.equal(a, b) for a, b in zip(once, (st.grad2d, st.count, st.max_radii)))


def test_bad_statistics_raise_at_forward_time(device):
    sc, cam = randscene_v1(500, 128, 128, ell=-3.0, seed=1, device=device)
    leaves = [sc[k] for k in NAMES]
    with pytest.raises(ValueError, match=r"\[500\]"):
        render_gaussians_trainable(*leaves, cam, densify=DensifyStats(499, device))
    with pytest.raises(ValueError, match="cpu"):
        render_gaussians_trainable(*leaves, cam, densify=DensifyStats(500, "cpu"))
    st = DensifyStats(500, device)
    st.count = torch.zeros(1000, device=device)[::2]
    with pytest.raises(ValueError, match="contiguous"):
        render_gaussians_trainable(*leaves, cam, densify=st)
