"""CPU: the definitions of the bilateral-grid slice and its TV loss (mojosplat_amd/bilagrid.py) pinned by gsplat's
grid_sample formulation and by closed forms, the backward formula the HIP kernels implement (csrc/bilagrid.hip) restated
in torch against autograd of the definition, and the host logic of the entry points (validation needs no GPU)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import mojosplat_amd as ms
from mojosplat_amd import _hip
from mojosplat_amd import bilagrid as BG
from mojosplat_amd.bilagrid import (bilagrid_identity, bilagrid_slice, bilagrid_slice_torch, bilagrid_tv_loss,
                                    bilagrid_tv_loss_torch)

GRAY = torch.tensor([0.299, 0.587, 0.114], dtype=torch.float64)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _grids(B, Gw, Gh, L, seed=0, dtype=torch.float64):
    g = bilagrid_identity(B, (Gw, Gh, L), requires_grad=False).to(dtype)
    return g + 0.3 * torch.randn(g.shape, generator=_gen(seed), dtype=dtype)


def _colours(B, H, W, seed=1, dtype=torch.float64):
    return torch.rand(B, H, W, 3, generator=_gen(seed), dtype=dtype) * 1.4 - 0.2


def _gray(img):
    return (img[..., 0] * 0.299 + img[..., 1] * 0.587) + img[..., 2] * 0.114


def _grid_sample_formulation(grids, img):
    """gsplat's slice: grid_sample at (x, y, gray) in [0, 1]^3 mapped to [-1, 1]^3, then the 3x4 product."""
    B, H, W, _ = img.shape
    x = (torch.arange(W, dtype=img.dtype) + 0.5) / W
    y = (torch.arange(H, dtype=img.dtype) + 0.5) / H
    xyz = torch.stack([x[None, None, :].expand(B, H, W), y[None, :, None].expand(B, H, W), _gray(img)], -1)
    A = F.grid_sample(grids, ((xyz - 0.5) * 2)[:, None], mode="bilinear", align_corners=True, padding_mode="border")
    A = A[:, :, 0].permute(0, 2, 3, 1).reshape(B, H, W, 3, 4)
    return (A[..., :3] * img[..., None, :]).sum(-1) + A[..., 3]


@pytest.mark.parametrize("B,H,W,Gw,Gh,L", [(2, 13, 17, 4, 5, 8), (1, 7, 9, 2, 2, 2), (1, 30, 50, 16, 16, 8)])
def test_definition_equals_the_grid_sample_formulation(B, H, W, Gw, Gh, L):
    grids = _grids(B, Gw, Gh, L).requires_grad_(True)
    img = _colours(B, H, W)
    img[0, 0] = 0.0                                  # black pixels: z = 0 exactly
    img.requires_grad_(True)
    v_out = torch.randn(B, H, W, 3, generator=_gen(2), dtype=torch.float64)
    out = bilagrid_slice_torch(grids, img)
    ref = _grid_sample_formulation(grids, img)
    vg, vi = torch.autograd.grad((out * v_out).sum(), (grids, img))
    rg, ri = torch.autograd.grad((ref * v_out).sum(), (grids, img))
    assert (out - ref).abs().max() <= 5e-14
    assert (vg - rg).abs().max() <= 5e-14
    z = _gray(img.detach()) * (L - 1)
    compared = ((z > 0) & (z < L - 1)) | (img.detach() == 0).all(-1)
    assert compared.float().mean() > 0.5 and compared[0, 0].all()
    assert ((vi - ri).abs().max(-1).values[compared]).max() <= 1e-13


def _two_band_colours(B, H, W, seed=3):
    """Colours whose gray lies in [0.05, 0.45] or [0.55, 0.95]: under L = 3 every z is at least 0.1 from a level."""
    c = torch.rand(B, H, W, 3, generator=_gen(seed), dtype=torch.float64) * 0.4 + 0.05
    c[:, ::2] += 0.5
    return c


def test_gradcheck_of_both_definitions():
    grids = _grids(1, 3, 2, 3, seed=4).requires_grad_(True)
    img = _two_band_colours(1, 5, 6).requires_grad_(True)
    z = _gray(img.detach()) * 2
    assert ((z - z.round()).abs() >= 0.05).all() and (z < 1).any() and (z > 1).any()
    assert torch.autograd.gradcheck(bilagrid_slice_torch, (grids, img), eps=1e-7, atol=1e-7)
    assert torch.autograd.gradcheck(bilagrid_tv_loss_torch, (grids,), eps=1e-7, atol=1e-7)
    assert torch.autograd.gradcheck(bilagrid_slice_torch, (grids[0], img[0]), eps=1e-7, atol=1e-7)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_identity_grid_returns_the_image(dtype):
    img = _colours(2, 11, 14, dtype=dtype)
    g = bilagrid_identity(2, (5, 4, 6), requires_grad=False).to(dtype)
    assert g.shape == (2, 12, 6, 4, 5) and bilagrid_identity(3).shape == (3, 12, 8, 16, 16)
    assert bilagrid_identity(1).dtype == torch.float32 and bilagrid_identity(1).requires_grad
    out = bilagrid_slice_torch(g, img)
    assert out.dtype == dtype and out.shape == img.shape
    assert (out - img).abs().max() <= 4 * torch.finfo(dtype).eps * 1.2
    assert float(bilagrid_tv_loss_torch(g)) == 0.0


def test_a_single_vertex_is_a_global_affine():
    img = _colours(1, 9, 10)
    A = torch.randn(3, 4, generator=_gen(5), dtype=torch.float64)
    g = A.reshape(1, 12, 1, 1, 1).clone().requires_grad_(True)
    x = img.clone().requires_grad_(True)
    out = bilagrid_slice_torch(g, x)
    assert (out - (img @ A[:, :3].T + A[:, 3])).abs().max() <= 1e-14
    v_out = torch.randn(1, 9, 10, 3, generator=_gen(6), dtype=torch.float64)
    vg, vx = torch.autograd.grad((out * v_out).sum(), (g, x))
    assert (vx - v_out @ A[:, :3]).abs().max() <= 1e-14                     # no guidance term: L = 1
    ones = torch.cat([img, torch.ones(1, 9, 10, 1, dtype=torch.float64)], -1)
    assert (vg.reshape(3, 4) - torch.einsum("bhwi,bhwj->ij", v_out, ones)).abs().max() <= 1e-12
    assert float(bilagrid_tv_loss_torch(g.detach())) == 0.0                 # three axes of size 1


def test_a_grid_constant_along_the_levels_has_no_guidance_gradient():
    base = _grids(1, 4, 3, 1, seed=7)
    g = base.expand(1, 12, 5, 3, 4).contiguous()
    img = _colours(1, 8, 9).requires_grad_(True)
    v_out = torch.randn(1, 8, 9, 3, generator=_gen(8), dtype=torch.float64)
    (vi,) = torch.autograd.grad((bilagrid_slice_torch(g, img) * v_out).sum(), (img,))
    (vi1,) = torch.autograd.grad((bilagrid_slice_torch(base, img) * v_out).sum(), (img,))   # L = 1: A^T v_out alone
    assert (vi - vi1).abs().max() <= 1e-14


@pytest.mark.parametrize("dim", [2, 3, 4])
def test_tv_of_a_linear_grid_and_size_one_axes(dim):
    d = 0.37
    shape = [3, 12, 6, 5, 4]
    idx = torch.arange(shape[dim], dtype=torch.float64).reshape([-1 if k == dim else 1 for k in range(5)])
    g = (d * idx).expand(shape).contiguous()
    assert abs(float(bilagrid_tv_loss_torch(g)) - d * d) <= 1e-14
    assert abs(float(bilagrid_tv_loss_torch(g[1])) - d * d) <= 1e-14       # a 4-D grid is a batch of one
    # an axis of size 1 contributes 0: the other two keep their own means
    r = _grids(2, 4, 5, 6, seed=9)
    one = r.narrow(dim, 0, 1)
    others = [k for k in (2, 3, 4) if k != dim]
    want = sum(((one.narrow(k, 1, one.shape[k] - 1) - one.narrow(k, 0, one.shape[k] - 1)) ** 2).mean() for k in others)
    assert abs(float(bilagrid_tv_loss_torch(one)) - float(want)) <= 1e-14


def _hat(t, n):
    """(...,) -> (..., n): the weight max(0, 1 - |clamp(t) - l|) of every vertex l of an axis."""
    tc = t.clamp(0, n - 1) if n > 1 else torch.zeros_like(t)
    return (1 - (tc[..., None] - torch.arange(n, dtype=t.dtype)).abs()).clamp(min=0)


@pytest.mark.parametrize("B,H,W,Gw,Gh,L", [(2, 13, 17, 4, 5, 8), (1, 9, 7, 1, 3, 2), (2, 6, 5, 3, 1, 1)])
def test_backward_formula_of_the_kernels_equals_autograd(B, H, W, Gw, Gh, L):
    """v_grids[b, c, l, gy, gx] = sum over pixels of hat_gy(v) hat_gx(u) hat_l(z) v_out_i (rgb_j or 1), and
    v_img = A^T v_out + [0 < z < L - 1] (L - 1) (sum_c (G[i0 + 1] - G[i0])_c g_c) (0.299, 0.587, 0.114): what k_slice_gather
    and k_slice_tile<true> compute."""
    grids = _grids(B, Gw, Gh, L, seed=10).requires_grad_(True)
    img = _colours(B, H, W, seed=11)
    img[0, 1] = 0.0
    img[0, 2] = 1.0
    img.requires_grad_(True)
    v_out = torch.randn(B, H, W, 3, generator=_gen(12), dtype=torch.float64)
    vg, vi = torch.autograd.grad((bilagrid_slice_torch(grids, img) * v_out).sum(), (grids, img))
    x, G = img.detach(), grids.detach()
    u = (torch.arange(W, dtype=torch.float64) + 0.5) / W * (Gw - 1)
    v = (torch.arange(H, dtype=torch.float64) + 0.5) / H * (Gh - 1)
    z = _gray(x) * (L - 1)
    Wx, Wy, Wz = _hat(u, Gw), _hat(v, Gh), _hat(z, L)
    gc = (v_out[..., :, None] * torch.cat([x, torch.ones(B, H, W, 1, dtype=torch.float64)], -1)[..., None, :]).reshape(B, H, W, 12)
    v_grids = torch.einsum("bhwl,hy,wx,bhwc->bclyx", Wz, Wy, Wx, gc)
    assert (v_grids - vg).abs().max() <= 1e-12
    A = torch.einsum("bhwl,hy,wx,bclyx->bhwc", Wz, Wy, Wx, G).reshape(B, H, W, 3, 4)
    v_img = torch.einsum("bhwij,bhwi->bhwj", A[..., :3], v_out)
    if L > 1:
        i0 = z.clamp(0, L - 1).floor().clamp(max=L - 2).long()
        Dz = F.one_hot(i0 + 1, L).double() - F.one_hot(i0, L).double()
        dA = torch.einsum("bhwl,hy,wx,bclyx->bhwc", Dz, Wy, Wx, G)
        inside = ((z > 0) & (z < L - 1)).double()
        v_img = v_img + (inside * (L - 1) * (dA * gc).sum(-1))[..., None] * GRAY
    assert (v_img - vi).abs().max() <= 1e-12
    # the TV gradient: 2 / count times (difference to the previous neighbour - difference to the next), per axis
    (tg,) = torch.autograd.grad(bilagrid_tv_loss_torch(grids), (grids,))
    want = torch.zeros_like(G)
    for dim in (2, 3, 4):
        n = G.shape[dim]
        if n >= 2:
            d = G.narrow(dim, 1, n - 1) - G.narrow(dim, 0, n - 1)
            k = 2.0 / (d.numel() // B) / B
            want.narrow(dim, 1, n - 1).add_(k * d)
            want.narrow(dim, 0, n - 1).sub_(k * d)
    assert (want - tg).abs().max() <= 1e-14


def test_library_exports_and_validates_the_bilagrid_entry_points():
    lib = _hip.load()
    for name in ("ms_bilagrid_slice_workspace_bytes", "ms_bilagrid_slice_fwd", "ms_bilagrid_slice_bwd",
                 "ms_bilagrid_tv_workspace_bytes", "ms_bilagrid_tv_fwd", "ms_bilagrid_tv_bwd"):
        assert hasattr(lib, name) and name in _hip.EXPORTS
    P = ctypes.c_void_p(0x1000)   # validation never dereferences it
    INVALID, WORKSPACE, TOO_LARGE = 1, 2, 3
    err = lambda: lib.ms_last_error_string().decode()
    wsb = lib.ms_bilagrid_slice_workspace_bytes
    need = wsb(1, 1080, 1920, 8, 16, 16)
    assert need > 0 and need % (16 * 16 * 8 * 12 * 4) == 0 and wsb(2, 1080, 1920, 8, 16, 16) == 2 * need
    assert wsb(1, 0, 1920, 8, 16, 16) == 0 and wsb(1, 1080, 1920, 0, 16, 16) == 0
    assert wsb(1, 1080, -1, 8, 16, 16) == 0 and wsb(-1, 1080, 1920, 8, 16, 16) == 0 and wsb(1, 1080, 1920, 8, 16, -2) == 0

    def fwd(B=1, H=1080, W=1920, L=8, Gh=16, Gw=16, grids=P, img=P, out=P):
        return lib.ms_bilagrid_slice_fwd(B, H, W, L, Gh, Gw, grids, img, out, None)

    def bwd(B=1, H=1080, W=1920, L=8, Gh=16, Gw=16, grids=P, img=P, v_out=P, ws=P, nbytes=need, v_grids=P, v_img=P):
        return lib.ms_bilagrid_slice_bwd(B, H, W, L, Gh, Gw, grids, img, v_out, ws, nbytes, v_grids, v_img, None)

    for f in (fwd, bwd):
        assert f(grids=None) == INVALID and "null" in err()
        assert f(img=None) == INVALID and "null" in err()
        assert f(H=0) == INVALID and "size" in err()
        assert f(W=-3) == INVALID and "size" in err()
        assert f(B=0) == INVALID and "size" in err()
        assert f(L=0) == INVALID and "size" in err()
        assert f(Gw=-1) == INVALID and "size" in err()
        assert f(H=1 << 24) == TOO_LARGE and "2^23" in err()
        assert f(B=4, L=1 << 12, Gh=1 << 12, Gw=1 << 12) == TOO_LARGE and "2^31" in err()
    assert fwd(out=None) == INVALID and "null" in err()
    assert bwd(v_out=None) == INVALID and "null" in err()
    assert bwd(ws=None) == INVALID and "null" in err()
    assert bwd(nbytes=need - 1) == WORKSPACE and "workspace" in err()

    tvb = lib.ms_bilagrid_tv_workspace_bytes
    tneed = tvb(200, 8, 16, 16)
    assert tneed > 0 and tvb(0, 8, 16, 16) == 0 and tvb(2, 8, 0, 16) == 0 and tvb(2, -8, 16, 16) == 0
    tv_fwd = lambda B=200, L=8, Gh=16, Gw=16, g=P, ws=P, n=tneed, out=P: lib.ms_bilagrid_tv_fwd(B, L, Gh, Gw, g, ws, n, out, None)
    tv_bwd = lambda B=200, L=8, Gh=16, Gw=16, g=P, vl=P, vg=P: lib.ms_bilagrid_tv_bwd(B, L, Gh, Gw, g, vl, vg, None)
    for f in (tv_fwd, tv_bwd):
        assert f(g=None) == INVALID and "null" in err()
        assert f(B=0) == INVALID and "size" in err()
        assert f(Gh=-4) == INVALID and "size" in err()
        assert f(B=4, L=1 << 12, Gh=1 << 12, Gw=1 << 12) == TOO_LARGE and "2^31" in err()
    assert tv_fwd(ws=None) == INVALID and tv_fwd(out=None) == INVALID
    assert tv_fwd(n=tneed - 1) == WORKSPACE and "workspace" in err()
    assert tv_bwd(vl=None) == INVALID and tv_bwd(vg=None) == INVALID


def test_public_names_and_what_the_hip_backend_refuses():
    for name in ("bilagrid_identity", "bilagrid_slice", "bilagrid_tv_loss", "bilagrid_slice_torch", "bilagrid_tv_loss_torch"):
        assert name in ms.__all__ and getattr(ms, name) is getattr(BG, name)
    g, img = _grids(2, 4, 3, 5, dtype=torch.float32), _colours(2, 6, 7, dtype=torch.float32)
    for backend in ("hip", "torch"):
        with pytest.raises(ValueError, match="expected grids"):
            bilagrid_slice(g, img[0], backend=backend)              # 5-D grids with a 3-D image
        with pytest.raises(ValueError, match="do not go together"):
            bilagrid_slice(g[:, :11], img, backend=backend)
        with pytest.raises(ValueError, match="do not go together"):
            bilagrid_slice(g, torch.cat([img, img[..., :1]], -1), backend=backend)   # C = 4
        with pytest.raises(ValueError, match="do not go together"):
            bilagrid_slice(g[:1], img, backend=backend)             # B differs
        with pytest.raises(ValueError, match="floating point"):
            bilagrid_slice(g, (img * 255).to(torch.uint8), backend=backend)
        with pytest.raises(ValueError, match="expected grids"):
            bilagrid_tv_loss(g[0, 0], backend=backend)
        with pytest.raises(ValueError, match="floating-point"):
            bilagrid_tv_loss(g.long(), backend=backend)
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        bilagrid_slice(g, img)                                      # "hip" is the default
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        bilagrid_slice(g[0], img[0], backend="hip")
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        bilagrid_tv_loss(g)
    with pytest.raises(ValueError, match="Invalid backend"):
        bilagrid_slice(g, img, backend="triton")
    with pytest.raises(ValueError, match="Invalid backend"):
        bilagrid_tv_loss(g, backend="numpy")
    with pytest.raises(ValueError):
        bilagrid_identity(2, (4, 0, 3))
    assert bilagrid_slice(g, img, backend="torch").shape == img.shape
    assert bilagrid_slice(g[0], img[0], backend="torch").shape == img[0].shape
    assert bilagrid_tv_loss(g, backend="torch").dim() == 0
