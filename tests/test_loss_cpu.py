"""CPU: the definition of the photometric loss (mojosplat_amd/loss.py) pinned by properties that do not depend on its
own code, the backward formula the HIP kernel implements (csrc/loss.hip) restated in torch against autograd of the
definition, and the host logic of the three entry points (argument validation needs no GPU)."""
import ctypes
import math

import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import _hip, photometric_loss
from mojosplat_amd import loss as L
from mojosplat_amd.loss import photometric_loss_torch, ssim_map_torch, ssim_torch

C1, C2 = 0.01 ** 2, 0.03 ** 2


def _rand(*shape, seed=0, dtype=torch.float64):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def _window():
    g = [math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)]
    s = sum(g)
    return [v / s for v in g]


def test_identical_images():
    x = _rand(40, 33, 3)
    assert abs(float(ssim_torch(x, x)) - 1.0) <= 1e-12
    assert float(photometric_loss_torch(x, x)) == pytest.approx(0.0, abs=1e-12)
    assert float((x - x).abs().mean()) == 0.0


def test_constant_images_closed_form_and_zero_padding():
    a, b = 0.3, 0.7
    x, y = torch.full((30, 28, 2), a, dtype=torch.float64), torch.full((30, 28, 2), b, dtype=torch.float64)
    m = ssim_map_torch(x, y)
    closed = (2 * a * b + C1) / (a * a + b * b + C1)
    assert (m[5:-5, 5:-5] - closed).abs().max() <= 1e-12
    for cy, cx in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        assert (m[cy, cx] - closed).abs().min() > 1e-3   # the padding's zeros are inside a corner pixel's window


def test_brute_force_121_taps():
    H, W, C = 23, 19, 3
    x, y = _rand(H, W, C, seed=1), _rand(H, W, C, seed=2)
    g = _window()
    ref = torch.zeros(H, W, C, dtype=torch.float64)
    for c in range(C):
        for i in range(H):
            for j in range(W):
                mx = my = exx = eyy = exy = 0.0
                for di in range(11):
                    for dj in range(11):
                        ii, jj = i + di - 5, j + dj - 5
                        if 0 <= ii < H and 0 <= jj < W:
                            w = g[di] * g[dj]
                            xv, yv = float(x[ii, jj, c]), float(y[ii, jj, c])
                            mx += w * xv
                            my += w * yv
                            exx += w * xv * xv
                            eyy += w * yv * yv
                            exy += w * xv * yv
                sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
                ref[i, j, c] = (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    assert (ssim_map_torch(x, y) - ref).abs().max() <= 1e-12


def test_symmetry_batch_and_shapes():
    x, y = _rand(3, 21, 34, 3, seed=3), _rand(3, 21, 34, 3, seed=4)
    assert abs(float(ssim_torch(x, y) - ssim_torch(y, x))) <= 1e-14
    assert torch.equal(ssim_map_torch(x[0], y[0]), ssim_map_torch(x[:1], y[:1])[0])
    assert float(photometric_loss_torch(x[0], y[0])) == float(photometric_loss_torch(x[:1], y[:1]))
    per = torch.stack([photometric_loss_torch(x[b], y[b]) for b in range(3)])
    assert abs(float(photometric_loss_torch(x, y) - per.mean())) <= 1e-14
    loss, l1, ssim_v = photometric_loss_torch(x, y, 0.35, return_parts=True)
    assert abs(float(loss) - (0.65 * float(l1) + 0.35 * (1 - float(ssim_v)))) <= 1e-14
    assert float(ms.ssim(x, y, backend="torch")) == float(ssim_v)
    assert photometric_loss_torch(x.float(), y.float()).dtype == torch.float32


def test_gradcheck_of_the_definition():
    x = _rand(13, 12, 2, seed=5).requires_grad_(True)
    y = _rand(13, 12, 2, seed=6).requires_grad_(True)
    assert (x - y).abs().min() > 1e-5
    assert torch.autograd.gradcheck(lambda a, b: photometric_loss_torch(a, b, 0.2), (x, y), eps=1e-7, atol=1e-7)


def _conv(t, w2d):
    C = t.shape[1]
    return torch.nn.functional.conv2d(t, w2d.expand(C, 1, 11, 11), padding=5, groups=C)


@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
def test_backward_formula_of_the_kernel_equals_autograd(lam):
    """v_x = v_loss ((1 - lambda) sign(x - y) / n - lambda / n (w*a + 2 x (w*b) + y (w*c))) with a = d ssim / d mu_x at
    fixed w*x^2 and w*xy, b = d ssim / d s_xx, c = d ssim / d s_xy: what k_loss_bwd computes from the forward's planes."""
    B, H, W, C = 2, 26, 31, 3
    x = _rand(B, H, W, C, seed=7).requires_grad_(True)
    y = _rand(B, H, W, C, seed=8)
    v_loss = 1.7
    (v_loss * photometric_loss_torch(x, y, lam)).backward()
    g = torch.tensor(_window(), dtype=torch.float64)
    w2d = g[:, None] * g[None, :]
    xn, yn = x.detach().permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    mx, my = _conv(xn, w2d), _conv(yn, w2d)
    sxx, syy, sxy = _conv(xn * xn, w2d) - mx * mx, _conv(yn * yn, w2d) - my * my, _conv(xn * yn, w2d) - mx * my
    A1, A2, B1, B2 = 2 * mx * my + C1, 2 * sxy + C2, mx * mx + my * my + C1, sxx + syy + C2
    ssim_map = A1 * A2 / (B1 * B2)
    b = -ssim_map / B2
    c = 2 * A1 / (B1 * B2)
    a = 2 * my * A2 / (B1 * B2) - 2 * mx * ssim_map / B1 - 2 * mx * b - my * c
    n = x.numel()
    v = v_loss * ((1 - lam) * torch.sign(xn - yn) / n - lam / n * (_conv(a, w2d) + 2 * xn * _conv(b, w2d) + yn * _conv(c, w2d)))
    assert (v.permute(0, 2, 3, 1) - x.grad).abs().max() <= 1e-10 * max(1.0, float(x.grad.abs().max()))
    assert (v.permute(0, 2, 3, 1) - x.grad).abs().max() <= 1e-10


def test_library_exports_and_validates_the_loss_entry_points():
    lib = _hip.load()
    for name in ("ms_photometric_loss_workspace_bytes", "ms_photometric_loss_fwd", "ms_photometric_loss_bwd"):
        assert hasattr(lib, name) and name in _hip.EXPORTS
    P = ctypes.c_void_p(0x1000)   # validation never dereferences it
    INVALID, WORKSPACE, TOO_LARGE = 1, 2, 3
    err = lambda: lib.ms_last_error_string().decode()
    wsb = lib.ms_photometric_loss_workspace_bytes
    small, kept = wsb(1, 100, 200, 3, 0), wsb(1, 100, 200, 3, 1)
    assert small > 0 and kept == small + 3 * 4 * 100 * 200 * 3
    assert wsb(1, 0, 200, 3, 1) == 0 and wsb(1, 100, 200, 5, 1) == 0 and wsb(0, 100, 200, 3, 0) == 0

    def fwd(B=1, H=100, W=200, C=3, img=P, tgt=P, lam=0.2, ws=P, nbytes=kept, keep=1, out=P):
        return lib.ms_photometric_loss_fwd(B, H, W, C, img, tgt, lam, ws, nbytes, keep, out, None)

    def bwd(B=1, H=100, W=200, C=3, img=P, tgt=P, lam=0.2, ws=P, nbytes=kept, v_loss=P, v_img=P):
        return lib.ms_photometric_loss_bwd(B, H, W, C, img, tgt, lam, ws, nbytes, v_loss, v_img, None)

    for f in (fwd, bwd):
        assert f(img=None) == INVALID and "null" in err()
        assert f(tgt=None) == INVALID and "null" in err()
        assert f(ws=None) == INVALID and "null" in err()
        assert f(H=0) == INVALID and "size" in err()
        assert f(W=-3) == INVALID and "size" in err()
        assert f(B=0) == INVALID and "size" in err()
        assert f(C=0) == INVALID and "channels" in err()
        assert f(C=5) == INVALID and "channels" in err()
        assert f(lam=-0.1) == INVALID and "lambda" in err()
        assert f(lam=1.5) == INVALID and "lambda" in err()
        assert f(lam=float("nan")) == INVALID and "lambda" in err()
        assert f(nbytes=kept - 1) == WORKSPACE and "workspace" in err()
        assert f(B=4, H=40000, W=40000, C=1) == TOO_LARGE and "2^31" in err()
    assert fwd(out=None) == INVALID and "null" in err()
    assert fwd(nbytes=small - 1, keep=0) == WORKSPACE
    assert bwd(nbytes=small) == WORKSPACE and "keep_for_backward" in err()   # a forward that kept nothing cannot feed a backward
    assert bwd(v_loss=None) == INVALID and bwd(v_img=None) == INVALID


def test_hip_backend_refuses_what_it_cannot_do():
    x, y = _rand(8, 9, 3, dtype=torch.float32), _rand(8, 9, 3, seed=1, dtype=torch.float32)
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        photometric_loss(x, y, backend="hip")
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        photometric_loss(x, y)                      # "hip" is the default
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        ms.ssim(x, y)
    with pytest.raises(ValueError, match='backend="torch"'):
        photometric_loss(x, y.clone().requires_grad_(True), backend="hip")
    with pytest.raises(ValueError, match="Invalid backend"):
        photometric_loss(x, y, backend="triton")
    with pytest.raises(ValueError, match="Invalid backend"):
        ms.ssim(x, y, backend="numpy")
    with pytest.raises(ValueError, match="lambda_dssim"):
        photometric_loss(x, y, lambda_dssim=1.2, backend="torch")
    with pytest.raises(ValueError, match="shape"):
        photometric_loss(x, y[:4], backend="torch")
    assert photometric_loss(x, y, backend="torch").dim() == 0
    assert "photometric_loss" in ms.__all__ and "ssim" in ms.__all__ and L.photometric_loss is photometric_loss
