"""GPU: the fused photometric loss (csrc/loss.hip; mojosplat_amd/loss.py, backend="hip") against its definition.

Values and gradients are held to the definition evaluated in float64 on the CPU, with a bar MEASURED per input against
the same definition in float32: e32 = |definition in float32 - definition in float64|, required
ehip <= 4 e32 + 4 eps32 |value| (the factor 4: a different order of the same float32 sums).  Largest pairs observed on
an MI355X: DESIGN.md, section "Photometric loss"."""
import os

import pytest
import torch

import mojosplat_amd as ms
from helpers import GOLDEN_DIR, _posed, assert_grad_close, camera_from_golden, load_golden
from mojosplat_amd import _hip, photometric_loss
from mojosplat_amd.autograd import render_gaussians_trainable
from mojosplat_amd.densify import DensifyStats
from mojosplat_amd.loss import photometric_loss_torch

pytestmark = pytest.mark.gpu

EPS32 = torch.finfo(torch.float32).eps
NAMES = ("means3d", "scales", "quats", "opacities", "features")


def _golden_scene(device):
    d, c = load_golden(os.path.join(GOLDEN_DIR, "randscene_n5000_640x360.npz"))
    cam = camera_from_golden(d, c, device)
    sc = {k: torch.from_numpy(d[k]).to(device) for k in ("means3d", "scales", "quats", "opacities")}
    sc["features"] = torch.from_numpy(d["colors"]).to(device)
    return sc, cam


def _perturbed(sc, seed=11):
    g = torch.Generator().manual_seed(seed)
    out = dict(sc)
    out["means3d"] = sc["means3d"] + 0.02 * torch.randn(sc["means3d"].shape, generator=g).to(sc["means3d"].device)
    out["features"] = (sc["features"] + 0.1 * torch.randn(sc["features"].shape, generator=g).to(sc["features"].device)).clamp(0, 1)
    return out


def _render(sc, cam):
    bg = torch.zeros(3, device=sc["means3d"].device)
    return ms.render_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"], cam,
                               background_color=bg, backend="hip")


def _inputs(kind, B, H, W, C, device, seed=0):
    """-> (x, y) float32 on the CPU, shape (H, W, C) when B == 1 else (B, H, W, C)."""
    g = torch.Generator().manual_seed(seed)
    shape = (H, W, C) if B == 1 else (B, H, W, C)
    if kind == "noise":
        return torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if kind == "smooth":
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        base = torch.stack([0.5 + 0.4 * torch.sin(0.031 * (c + 1) * xx + 0.5 * c) * torch.cos(0.023 * (c + 2) * yy)
                            for c in range(C)], -1)
        base = base.expand(shape).contiguous()
        return base, base + 0.02 * torch.randn(shape, generator=g)
    if kind == "same":
        x = torch.rand(shape, generator=g)
        return x, x.clone()
    assert kind == "render" and (B, C) == (1, 3)
    sc, cam = _golden_scene(device)
    assert (cam.H, cam.W) == (H, W)
    x, y = _render(_perturbed(sc), cam).cpu(), _render(sc, cam).cpu()
    print(f"\n[loss render] exactly-zero share of the target: {float((y == 0).float().mean()):.3f}")
    return x, y


CASES = [  # kind, B, H, W, C
    ("noise", 1, 170, 250, 3), ("noise", 3, 37, 53, 1), ("noise", 1, 1, 1, 3), ("noise", 1, 5, 300, 4),
    ("noise", 3, 53, 37, 4), ("noise", 1, 1080, 1920, 3),
    ("smooth", 1, 170, 250, 3), ("smooth", 3, 37, 53, 4), ("smooth", 1, 5, 300, 1), ("smooth", 1, 1080, 1920, 3),
    ("render", 1, 360, 640, 3),
    ("same", 1, 170, 250, 3), ("same", 3, 37, 53, 1), ("same", 1, 1, 1, 4), ("same", 1, 5, 300, 3),
    ("same", 1, 1080, 1920, 3),
]
IDS = ["%s-B%d-%dx%dx%d" % c for c in CASES]


def _definition(x, y, lam, dtype):
    """(triple, gradient) of the definition on the CPU in `dtype`."""
    xd = x.detach().clone().to(dtype).requires_grad_(True)
    loss, l1, ssim_v = photometric_loss_torch(xd, y.to(dtype), lam, return_parts=True)
    loss.backward()
    return torch.stack([loss.detach(), l1, ssim_v]).double(), xd.grad.double()


def _run_hip(x, y, lam, device, v_scale=None):
    xg = x.detach().clone().to(device).requires_grad_(True)
    loss, l1, ssim_v = photometric_loss(xg, y.to(device), lam, backend="hip", return_parts=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device == xg.device
    assert not l1.requires_grad and not ssim_v.requires_grad
    (loss if v_scale is None else v_scale * loss + 1).backward()
    return torch.stack([loss.detach(), l1, ssim_v]).cpu(), xg.grad.cpu()


@pytest.mark.parametrize("kind,B,H,W,C", CASES, ids=IDS)
def test_value_and_gradient_against_the_float64_definition(device, kind, B, H, W, C):
    lam = 0.2
    x, y = _inputs(kind, B, H, W, C, device)
    v64, g64 = _definition(x, y, lam, torch.float64)
    v32, g32 = _definition(x, y, lam, torch.float32)
    vh, gh = _run_hip(x, y, lam, device)
    vh, gh = vh.double(), gh.double()
    # 1. value
    e32, ehip = (v32 - v64).abs(), (vh - v64).abs()
    print(f"\n[loss {kind} B{B} {H}x{W}x{C}] value: e32 = {e32.tolist()} ehip = {ehip.tolist()} (loss, l1, ssim = {v64.tolist()})")
    # 2. gradient
    n2 = lambda t: float(t.norm())
    r32, rhip, ref = n2(g32 - g64), n2(gh - g64), n2(g64)
    m32, mhip, mref = float((g32 - g64).abs().max()), float((gh - g64).abs().max()), float(g64.abs().max())
    print(f"[loss {kind} B{B} {H}x{W}x{C}] gradient: |g64|_2 = {ref:.6g} L2 err f32 = {r32:.6g} hip = {rhip:.6g}; "
          f"max err f32 = {m32:.6g} hip = {mhip:.6g} (max|g64| = {mref:.6g})")
    assert gh.shape == x.shape and torch.isfinite(gh).all()
    for k, name in enumerate(("loss", "l1", "ssim")):
        assert float(ehip[k]) <= 4 * float(e32[k]) + 4 * EPS32 * abs(float(v64[k])), \
            f"{name}: ehip {float(ehip[k]):.3g} > 4 * e32 {float(e32[k]):.3g} + 4 eps |{float(v64[k]):.6g}|"
    if kind == "same":
        assert float(vh[1]) == 0.0
        assert abs(float(vh[2]) - 1.0) <= 4 * EPS32 + 4 * float(e32[2])
    # (the relative-L2 rule of the issue, multiplied through by |g64|_2 so that a vanishing gradient is no 0 / 0)
    assert rhip <= 4 * r32 + 4 * EPS32 * ref, f"gradient L2: hip {rhip:.3g} > 4 * f32 {r32:.3g} + 4 eps * {ref:.3g}"
    assert mhip <= 4 * m32 + 4 * EPS32 * mref, f"gradient max: hip {mhip:.3g} > 4 * f32 {m32:.3g} + 4 eps * {mref:.3g}"


def test_upstream_gradient_and_the_two_ends_of_lambda(device):
    x, y = _inputs("noise", 1, 170, 250, 3, device, seed=3)
    y[:7, :9] = x[:7, :9]                         # some exact ties: sign(0) = 0
    _, g1 = _run_hip(x, y, 0.2, device)
    _, g35 = _run_hip(x, y, 0.2, device, v_scale=3.5)
    assert ((g35.double() - 3.5 * g1.double()).abs() <= EPS32 * (3.5 * g1.double()).abs()).all()   # one rounding per element
    n = x.numel()
    _, g0 = _run_hip(x, y, 0.0, device)
    assert torch.equal(g0, (torch.sign(x.double() - y.double()) / n).float())
    assert (g0[:7, :9] == 0).all()
    # lambda = 1: no L1 part -- the gradient is that of -ssim alone, held to the definition at lambda = 1 by the gradient rule
    v64, g64 = _definition(x, y, 1.0, torch.float64)
    v32, g32 = _definition(x, y, 1.0, torch.float32)
    vh, gl = _run_hip(x, y, 1.0, device)
    assert float((gl.double() - g64).norm()) <= 4 * float((g32 - g64).norm()) + 4 * EPS32 * float(g64.norm())
    assert abs(float(vh[0]) - (1 - float(vh[2]))) <= 2 * EPS32
    # and an L1 part would show as a jump of 1 / n across a tie: at lambda = 1 the tied pixels carry the SSIM term alone
    assert (gl[:7, :9].double() - g64[:7, :9]).abs().max() <= 4 * float((g32 - g64).abs().max()) + 4 * EPS32 * float(g64.abs().max())


def test_bitwise_reproducible_also_on_another_stream(device):
    x, y = _inputs("noise", 3, 170, 250, 3, device, seed=5)
    v1, g1 = _run_hip(x, y, 0.2, device)
    v2, g2 = _run_hip(x, y, 0.2, device)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        v3, g3 = _run_hip(x, y, 0.2, device)
    side.synchronize()
    assert torch.equal(v1, v3) and torch.equal(g1, g3)


def test_no_hidden_copies_and_no_host_wait(device):
    B, H, W, C = 2, 540, 960, 3
    x = torch.rand(B, H, W, C, device=device)
    y = torch.rand(B, H, W, C, device=device)
    n = x.numel()
    ws_bytes = _hip.lib().ms_photometric_loss_workspace_bytes(B, H, W, C, 1)
    assert ws_bytes >= 12 * n
    photometric_loss(x[:1].clone().requires_grad_(True), y[:1]).backward()     # code objects loaded, allocator warm
    xg = x.requires_grad_(True)
    torch.cuda.synchronize(device)
    torch.cuda.reset_peak_memory_stats(device)
    base = torch.cuda.memory_allocated(device)
    loss = photometric_loss(xg, y)
    loss.backward()
    torch.cuda.synchronize(device)
    rise = torch.cuda.max_memory_allocated(device) - base
    print(f"\n[loss memory] rise {rise} B, gradient {4 * n} B + workspace {ws_bytes} B")
    assert rise <= 4 * n + ws_bytes + (1 << 20)
    assert xg.grad is not None and xg.grad.shape == x.shape
    # the forward returns without waiting for the device
    torch.cuda.set_sync_debug_mode("error")
    try:
        l2 = photometric_loss(xg, y)
        s2 = ms.ssim(x.detach(), y)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(l2.detach(), loss.detach()) and 0 < float(s2) < 1


def test_layouts_give_the_same_numbers(device):
    x, y = _inputs("noise", 1, 170, 250, 3, device, seed=9)
    y = y.half().float()                          # exactly representable in float16
    v, g = _run_hip(x, y, 0.2, device)
    v16, g16 = _run_hip(x, y.half(), 0.2, device)
    assert torch.equal(v, v16) and torch.equal(g, g16)
    big = torch.rand(190, 270, 3, generator=torch.Generator().manual_seed(1))
    big[10:180, 12:262] = y
    xg = x.to(device).requires_grad_(True)
    crop = big.to(device)[10:180, 12:262]
    assert not crop.is_contiguous()
    loss = photometric_loss(xg, crop)
    loss.backward()
    assert torch.equal(loss.detach().cpu(), v[0]) and torch.equal(xg.grad.cpu(), g)
    # a batch: the mean of its entries' values; its gradient the entries' own over B
    xb, yb = _inputs("noise", 3, 37, 53, 3, device, seed=2)
    vb, gb = _run_hip(xb, yb, 0.2, device)
    singles = [_run_hip(xb[b], yb[b], 0.2, device) for b in range(3)]
    assert abs(float(vb[0]) - sum(float(s[0][0]) for s in singles) / 3) <= 4 * EPS32
    for b in range(3):
        assert (gb[b] - singles[b][1] / 3).abs().max() <= 8 * EPS32 * singles[b][1].abs().max() / 3
    # the evaluation metric is the same forward
    assert torch.equal(ms.ssim(x.to(device), y.to(device)).cpu(), v[2])
    with torch.no_grad():
        assert torch.equal(photometric_loss(xg, y.to(device)).cpu(), v[0])
    with pytest.raises(ValueError, match='backend="torch"'):
        photometric_loss(xg, y.to(device).requires_grad_(True))
    with pytest.raises(_hip.HipBackendError, match="channels"):
        photometric_loss(torch.rand(8, 8, 5, device=device), torch.rand(8, 8, 5, device=device))


def _step(sc, cam, target, backend, bg):
    dev = target.device
    leaves = [sc[k].clone().requires_grad_(True) for k in NAMES]
    stats = DensifyStats(leaves[0].shape[0], dev)
    pcam = _posed(cam)
    img = render_gaussians_trainable(*leaves, pcam, background_color=bg, densify=stats)
    loss = photometric_loss(img, target, backend=backend)
    loss.backward()
    torch.cuda.synchronize(dev)
    return loss.detach(), [l.grad for l in leaves], stats, pcam.view_matrix.grad


def test_end_to_end_gradients_statistics_and_pose_match_the_torch_loss(device):
    sc, cam = _golden_scene(device)
    bg = torch.zeros(3, device=device)
    target = _render(_perturbed(sc), cam)
    lh, gh, sh, ph = _step(sc, cam, target, "hip", bg)
    lt, gt, st, pt = _step(sc, cam, target, "torch", bg)
    assert abs(float(lh) - float(lt)) <= 1e-5 * abs(float(lt))
    for name, a, b in zip(NAMES, gh, gt):
        assert b.abs().max() > 0
        assert_grad_close(f"loss-e2e/{name}", a, b)
    assert torch.equal(sh.count, st.count) and torch.equal(sh.max_radii, st.max_radii)
    assert_grad_close("loss-e2e/grad2d", sh.grad2d, st.grad2d)
    assert ph is not None and pt.abs().max() > 0
    assert_grad_close("loss-e2e/viewmat", ph, pt)


def test_twenty_adam_steps_halve_the_loss(device):
    sc, cam = _golden_scene(device)
    bg = torch.zeros(3, device=device)
    target = _render(sc, cam)
    g = torch.Generator().manual_seed(4)
    colors = torch.rand(sc["features"].shape, generator=g).to(device).requires_grad_(True)
    logit_op = torch.zeros_like(sc["opacities"]).requires_grad_(True)
    opt = torch.optim.Adam([colors, logit_op], lr=0.05)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        img = render_gaussians_trainable(sc["means3d"], sc["scales"], sc["quats"], torch.sigmoid(logit_op), colors, cam,
                                         background_color=bg)
        loss = photometric_loss(img, target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("\n[loss adam]", ["%.4f" % v for v in losses])
    assert losses[-1] < 0.5 * losses[0]
