"""GPU: the bilateral-grid slice and TV loss (csrc/bilagrid.hip; mojosplat_amd/bilagrid.py, backend="hip") against their
definitions.

The bar is the project's own (tests/test_hip_loss.py): for out, v_grids and v_img, in the L2 and in the maximum norm,
e_hip <= 4 e32 + 4 eps32 |value|, with e_hip the distance of the HIP result from the definition evaluated in float64 on
the CPU and e32 the distance of the definition in float32 on the CPU from the same (the factor 4: a different order of the
same float32 sums).  v_img alone is discontinuous in the guidance across a level: its comparison leaves out the pixels
whose float64 z lies within 1e-4 of an integer in [0, L - 1] (L > 1: with one level nothing depends on the guidance),
unless the pixel is exactly black -- black pixels are always compared -- and the left-out share is asserted to be at most
1 %.  The planted run of exact ones sits on z = L - 1 and is left out of v_img by that rule, so it is a whole row only where
a row is under 0.5 % of the pixels, and a shorter run otherwise (5 x 300: 7 pixels; 1 x 1: none); the run of exact zeros is
planted the same way.  Largest (e_hip, e32) pairs observed on an MI355X: DESIGN.md, section 4j."""
import os

import pytest
import torch

import mojosplat_amd as ms
from helpers import GOLDEN_DIR, assert_grad_close, camera_from_golden, load_golden
from mojosplat_amd import _hip, bilagrid_identity, bilagrid_slice, bilagrid_tv_loss, photometric_loss
from mojosplat_amd.autograd import render_gaussians_trainable
from mojosplat_amd.bilagrid import bilagrid_slice_torch, bilagrid_tv_loss_torch
from mojosplat_amd.optim import GaussianAdam

pytestmark = pytest.mark.gpu

EPS32 = torch.finfo(torch.float32).eps
NAMES = ("means3d", "scales", "quats", "opacities", "features")

CASES = [  # B, H, W, Gw, Gh, L
    (1, 1, 1, 2, 2, 2),          # a 1x1 image
    (3, 37, 53, 16, 16, 8),      # cells smaller than a tile (vertices from global memory); ragged tiles; three grids
    (1, 170, 250, 4, 3, 8),      # tiles inside one cell, and tiles straddling a cell edge
    (1, 5, 300, 2, 1, 2),        # Gh = 1
    (2, 37, 53, 1, 1, 1),        # the global affine
    (1, 64, 64, 16, 16, 1),      # L = 1
    (1, 1080, 1920, 16, 16, 8),  # once only
]
IDS = ["B%d-%dx%d-grid%dx%dx%d" % c for c in CASES]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _random_grids(B, Gw, Gh, L, seed=0):
    g = bilagrid_identity(B, (Gw, Gh, L), requires_grad=False)
    return g + 0.3 * torch.randn(g.shape, generator=_gen(seed))


def _colours(B, H, W, seed=1):
    """Uniform in [-0.2, 1.2] with a run of exact zeros and one of exact ones (module docstring) -> float32 (B, H, W, 3)."""
    img = torch.rand(B, H, W, 3, generator=_gen(seed)) * 1.4 - 0.2
    run = min(W, int(0.005 * B * H * W))
    if H >= 3 and run > 0:
        img[0, H // 3, :run] = 0.0
        img[0, 2 * H // 3, :run] = 1.0
    return img


def _gray(img):
    return (img[..., 0] * 0.299 + img[..., 1] * 0.587) + img[..., 2] * 0.114


def _golden_scene(device):
    d, c = load_golden(os.path.join(GOLDEN_DIR, "randscene_n5000_640x360.npz"))
    cam = camera_from_golden(d, c, device)
    sc = {k: torch.from_numpy(d[k]).to(device) for k in ("means3d", "scales", "quats", "opacities")}
    sc["features"] = torch.from_numpy(d["colors"]).to(device)
    return sc, cam


def _render(sc, cam):
    bg = torch.zeros(3, device=sc["means3d"].device)
    return ms.render_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"], cam,
                               background_color=bg, backend="hip")


def _definition(grids, img, v_out, dtype):
    """(out, v_grids, v_img) of the definition on the CPU in `dtype`, as float64."""
    g = grids.detach().clone().to(dtype).requires_grad_(True)
    x = img.detach().clone().to(dtype).requires_grad_(True)
    out = bilagrid_slice_torch(g, x)
    out.backward(v_out.to(dtype))
    return out.detach().double(), g.grad.double(), x.grad.double()


def _run_hip(grids, img, v_out, device):
    g = grids.detach().clone().to(device).requires_grad_(True)
    x = img.detach().clone().to(device).requires_grad_(True)
    out = bilagrid_slice(g, x, backend="hip")
    assert out.shape == x.shape and out.dtype == torch.float32 and out.device == x.device
    out.backward(v_out.to(device))
    assert g.grad.shape == g.shape and x.grad.shape == x.shape
    return out.detach().cpu(), g.grad.cpu(), x.grad.cpu()


def _hold(tag, name, hip, r32, r64, sel=None):
    """e_hip <= 4 e32 + 4 eps32 |value| in the L2 and in the maximum norm (over the elements `sel`, or all)."""
    hip = hip.double()
    assert hip.shape == r64.shape and torch.isfinite(hip).all()
    if sel is not None:
        hip, r32, r64 = hip[sel], r32[sel], r64[sel]
    if r64.numel() == 0:
        return
    for norm, f in (("L2", lambda t: float(t.norm())), ("max", lambda t: float(t.abs().max()))):
        e_hip, e32, ref = f(hip - r64), f(r32 - r64), f(r64)
        print(f"[bilagrid {tag}] {name} {norm}: e_hip = {e_hip:.6g} e32 = {e32:.6g} |value| = {ref:.6g}")
        assert e_hip <= 4 * e32 + 4 * EPS32 * ref, \
            f"{tag} {name} {norm}: e_hip {e_hip:.3g} > 4 * e32 {e32:.3g} + 4 eps * {ref:.3g}"


def _compared_pixels(img, L):
    """The pixels whose v_img is compared -> (bool mask of the image's leading shape, left-out share)."""
    x = img.double()
    black = (x == 0).all(-1)
    if L == 1:
        return torch.ones_like(black), 0.0
    z = _gray(x) * (L - 1)
    near = ((z - z.round()).abs() <= 1e-4) & (z.round() >= 0) & (z.round() <= L - 1)
    keep = ~near | black
    return keep, 1.0 - float(keep.double().mean())


def _check_case(tag, grids, img, v_out, L, device):
    r64 = _definition(grids, img, v_out, torch.float64)
    r32 = _definition(grids, img, v_out, torch.float32)
    hip = _run_hip(grids, img, v_out, device)
    print()
    _hold(tag, "out", hip[0], r32[0], r64[0])
    _hold(tag, "v_grids", hip[1], r32[1], r64[1])
    keep, left_out = _compared_pixels(img, L)
    print(f"[bilagrid {tag}] v_img: left-out share {left_out:.3g}, exactly black share {float((img == 0).all(-1).float().mean()):.3g}")
    assert left_out <= 0.01
    _hold(tag, "v_img", hip[2], r32[2], r64[2], sel=keep)
    return hip, r64


@pytest.mark.parametrize("B,H,W,Gw,Gh,L", CASES, ids=IDS)
def test_slice_and_gradients_against_the_float64_definition(device, B, H, W, Gw, Gh, L):
    grids, img = _random_grids(B, Gw, Gh, L), _colours(B, H, W)
    v_out = torch.randn(B, H, W, 3, generator=_gen(2))
    _check_case("B%d %dx%d %dx%dx%d" % (B, H, W, Gw, Gh, L), grids, img, v_out, L, device)


def test_render_of_the_golden_scene_on_black(device):
    sc, cam = _golden_scene(device)
    img = _render(sc, cam).cpu()[None]
    assert img.shape == (1, 360, 640, 3)
    black = float((img == 0).all(-1).float().mean())
    print(f"\n[bilagrid render] exactly black share {black:.3f}")
    assert black > 0.05
    grids = _random_grids(1, 16, 16, 8, seed=3)
    v_out = torch.randn(1, 360, 640, 3, generator=_gen(4))
    hip, r64 = _check_case("render 360x640 16x16x8", grids, img, v_out, 8, device)
    # 4-D grids with a 3-D image, and a crop that is not contiguous: the same numbers
    g = grids[0].to(device).requires_grad_(True)
    wide = torch.zeros(360, 650, 3, device=device)
    wide[:, 5:645] = img[0].to(device)
    x = wide[:, 5:645].requires_grad_(True)
    assert not x.is_contiguous()
    out = bilagrid_slice(g, x)
    out.backward(v_out[0].to(device))
    assert torch.equal(out.detach().cpu(), hip[0][0]) and torch.equal(g.grad.cpu(), hip[1][0])
    assert torch.equal(x.grad.cpu(), hip[2][0])


def test_exact_zeros(device):
    B, H, W, Gw, Gh, L = 1, 60, 70, 4, 3, 8
    grids = _random_grids(B, Gw, Gh, L, seed=5)
    img = torch.rand(B, H, W, 3, generator=_gen(6)) * 0.1 + 0.1       # gray in [0.1, 0.2]: z in [0.7, 1.4]
    z = _gray(img) * (L - 1)
    assert z.min() > 0.69 and z.max() < 1.41 and (z < 1).any() and (z > 1).any()
    v_out = torch.randn(B, H, W, 3, generator=_gen(7))
    _, vg, _ = _run_hip(grids, img, v_out, device)
    assert (vg[:, :, 3:] == 0).all()
    assert (vg[:, :, :3] != 0).all()
    # black pixels pass nothing through the guidance: v_img there is A^T v_out, A from level 0 alone
    img = _colours(1, 170, 250, seed=8)
    img[0, 11:14, 30:200] = 0.0
    black = (img == 0).all(-1)
    assert int(black.sum()) >= 3 * 170
    grids = _random_grids(1, 4, 3, 8, seed=9)
    v_out = torch.randn(1, 170, 250, 3, generator=_gen(10))
    _, _, vi = _run_hip(grids, img, v_out, device)
    level0 = grids[:, :, :1].double()

    def a_transpose_v(g, v):
        x = img.double().requires_grad_(True)
        bilagrid_slice_torch(g, x).backward(v)
        return x.grad

    want, bound = a_transpose_v(level0, v_out.double()), a_transpose_v(level0.abs(), v_out.double().abs())
    err = (vi.double() - want).abs()
    assert (err[black] <= 8 * EPS32 * bound[black]).all(), float((err[black] / bound[black]).max())
    # (and the guidance term is not small here: next to it, non-black pixels differ from A^T v_out by far more)
    assert float(err[~black].max()) > 1e-2


def test_bitwise_reproducible_also_on_another_stream(device):
    B, H, W, Gw, Gh, L = 2, 170, 250, 16, 16, 8
    grids, img = _random_grids(B, Gw, Gh, L, seed=11), _colours(B, H, W, seed=12)
    v_out = torch.randn(B, H, W, 3, generator=_gen(13))

    def tv():
        g = grids.to(device).requires_grad_(True)
        t = bilagrid_tv_loss(g)
        (3.0 * t).backward()
        return t.detach().cpu(), g.grad.cpu()

    a, ta = _run_hip(grids, img, v_out, device), tv()
    b, tb = _run_hip(grids, img, v_out, device), tv()
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        c, tc = _run_hip(grids, img, v_out, device), tv()
    side.synchronize()
    for other in (b + tb, c + tc):
        for u, v in zip(a + ta, other):
            assert torch.equal(u, v)


TV_CASES = [(1, 1, 1, 1), (3, 8, 5, 4), (2, 2, 16, 16), (200, 8, 16, 16)]     # B, L, Gh, Gw


@pytest.mark.parametrize("B,L,Gh,Gw", TV_CASES, ids=["B%d-%dx%dx%d" % c for c in TV_CASES])
def test_tv_loss_against_the_float64_definition(device, B, L, Gh, Gw):
    grids = _random_grids(B, Gw, Gh, L, seed=14)

    def definition(dtype):
        g = grids.clone().to(dtype).requires_grad_(True)
        t = bilagrid_tv_loss_torch(g)
        (1.7 * t).backward()
        return t.detach().double(), g.grad.double()

    (t64, g64), (t32, g32) = definition(torch.float64), definition(torch.float32)
    g = grids.to(device).requires_grad_(True)
    t = bilagrid_tv_loss(g)
    assert t.dim() == 0 and t.dtype == torch.float32 and t.device == g.device
    (1.7 * t).backward()
    tag = "tv B%d %dx%dx%d" % (B, L, Gh, Gw)
    print()
    _hold(tag, "value", t.detach().cpu().reshape(1), t32.reshape(1), t64.reshape(1))
    _hold(tag, "gradient", g.grad.cpu(), g32, g64)
    if (L, Gh, Gw) == (1, 1, 1):
        assert float(t.detach()) == 0.0 and (g.grad == 0).all()


def test_tv_of_identity_grids_and_odd_widths(device):
    g = bilagrid_identity(5, device=device)
    t = bilagrid_tv_loss(g)
    t.backward()
    assert float(t.detach()) == 0.0 and (g.grad == 0).all()
    # a width that is no multiple of 4 (one element per lane) and a base that is not 16-byte aligned
    for grids in (_random_grids(2, 7, 5, 3, seed=15), _random_grids(3, 8, 4, 2, seed=16)[1:]):
        gd = grids.to(device)
        if grids.shape[-1] == 8:
            flat = torch.empty(gd.numel() + 1, device=device)
            flat[1:] = gd.reshape(-1)
            gd = flat[1:].view(gd.shape)
            assert gd.data_ptr() % 16 != 0 and gd.is_contiguous()
        gd.requires_grad_(True)
        t = bilagrid_tv_loss(gd)
        t.backward()
        g64 = grids.double().requires_grad_(True)
        t64 = bilagrid_tv_loss_torch(g64)
        t64.backward()
        assert abs(float(t.detach()) - float(t64.detach())) <= 8 * EPS32 * float(t64.detach())
        assert (gd.grad.cpu().double() - g64.grad).abs().max() <= 16 * EPS32 * float(g64.grad.abs().max())


def test_requires_grad_combinations(device):
    B, H, W, Gw, Gh, L = 1, 270, 480, 16, 16, 8
    grids, img = _random_grids(B, Gw, Gh, L, seed=17).to(device), _colours(B, H, W, seed=18).to(device)
    v_out = torch.randn(B, H, W, 3, generator=_gen(19)).to(device)
    g, x = grids.clone().requires_grad_(True), img.clone().requires_grad_(True)
    out = bilagrid_slice(g, x)
    out.backward(v_out)
    g1 = grids.clone().requires_grad_(True)
    o1 = bilagrid_slice(g1, img)
    o1.backward(v_out)
    x2 = img.clone().requires_grad_(True)
    o2 = bilagrid_slice(grids, x2)
    o2.backward(v_out)
    assert torch.equal(o1, out) and torch.equal(o2, out)
    assert torch.equal(g1.grad, g.grad) and torch.equal(x2.grad, x.grad)
    o3 = bilagrid_slice(grids, img)
    assert not o3.requires_grad and o3.grad_fn is None and torch.equal(o3, out.detach())
    assert not bilagrid_tv_loss(grids).requires_grad
    # under no_grad the call keeps nothing and allocates no workspace: the result is all that memory rises by
    assert _hip.lib().ms_bilagrid_slice_workspace_bytes(B, H, W, L, Gh, Gw) > (64 << 10)
    torch.cuda.synchronize(device)
    torch.cuda.reset_peak_memory_stats(device)
    base = torch.cuda.memory_allocated(device)
    with torch.no_grad():
        o4 = bilagrid_slice(g, x)
    torch.cuda.synchronize(device)
    rise = torch.cuda.max_memory_allocated(device) - base
    print(f"\n[bilagrid memory] rise {rise} B, the result {4 * o4.numel()} B")
    assert o4.grad_fn is None and torch.equal(o4, out.detach())
    assert rise <= 4 * o4.numel() + (16 << 10)
    for bad in (grids.double(), grids.half()):
        with pytest.raises(ValueError, match="float32"):
            bilagrid_slice(bad, img)
        with pytest.raises(ValueError, match="float32"):
            bilagrid_tv_loss(bad)
    with pytest.raises(ValueError, match="the image on cpu"):
        bilagrid_slice(grids, img.cpu())
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        bilagrid_slice(grids.cpu(), img.cpu())


def _step(sc, cam, grids0, target, backend, bg):
    leaves = [sc[k].clone().requires_grad_(True) for k in NAMES]
    grids = grids0.clone().requires_grad_(True)
    img = render_gaussians_trainable(*leaves, cam, background_color=bg)
    img = bilagrid_slice(grids[1], img, backend=backend)
    loss = photometric_loss(img, target) + 10.0 * bilagrid_tv_loss(grids, backend=backend)
    loss.backward()
    torch.cuda.synchronize(target.device)
    return loss.detach(), [l.grad for l in leaves], grids.grad


def test_end_to_end_gradients_match_the_torch_definitions(device):
    sc, cam = _golden_scene(device)
    bg = torch.zeros(3, device=device)
    target = _render(sc, cam) * 0.8 + 0.05
    grids0 = _random_grids(3, 16, 16, 8, seed=20).to(device)
    lh, gh, vh = _step(sc, cam, grids0, target, "hip", bg)
    lt, gt, vt = _step(sc, cam, grids0, target, "torch", bg)
    assert abs(float(lh) - float(lt)) <= 1e-5 * abs(float(lt))
    for name, a, b in zip(NAMES, gh, gt):
        assert b.abs().max() > 0
        assert_grad_close(f"bilagrid-e2e/{name}", a, b)
    assert vt[1].abs().max() > 0 and vt[0].abs().max() > 0
    assert_grad_close("bilagrid-e2e/grids", vh, vt)


def test_twenty_steps_of_two_optimisers_bring_the_loss_down(device):
    sc, cam = _golden_scene(device)
    bg = torch.zeros(3, device=device)
    A = torch.tensor([[0.80, 0.10, 0.00, 0.03], [0.05, 0.90, 0.05, -0.02], [0.00, 0.15, 0.70, 0.04]], device=device)
    ref = _render(sc, cam)
    target = ref @ A[:, :3].T + A[:, 3]                       # a fixed non-identity affine of the reference render
    colors = sc["features"].clone().requires_grad_(True)
    grids = bilagrid_identity(2, device=device)
    opt = GaussianAdam({"features": colors}, lr=2e-3)
    grid_opt = GaussianAdam({"bilagrid": grids}, lr=5e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        grid_opt.zero_grad()
        img = render_gaussians_trainable(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], colors, cam,
                                         background_color=bg)
        loss = photometric_loss(bilagrid_slice(grids[0], img), target) + 10.0 * bilagrid_tv_loss(grids)
        loss.backward()
        opt.step()
        grid_opt.step()
        losses.append(float(loss.detach()))
    print("\n[bilagrid adam]", ["%.4f" % v for v in losses])
    assert losses[-1] < losses[0]
    assert grids.grad[1].abs().max() == 0                     # the view that was not rendered: no slice term, identity TV
