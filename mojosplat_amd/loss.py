"""The photometric loss of 3D Gaussian Splatting training: ``(1 - lambda) * L1 + lambda * (1 - SSIM)``.

Kerbl et al.'s trainer (and gsplat's) scores a render against its target with the mean absolute
difference and the structural similarity under an 11x11 Gaussian window (sigma 1.5, zero padding).
``photometric_loss_torch`` is the definition, in plain torch (any device, any float dtype,
differentiable in both images); ``photometric_loss(..., backend="hip")`` is the fused forward and
backward of csrc/loss.hip on the ``(H, W, C)`` image ``render_gaussians_trainable`` returns::

    img = render_gaussians_trainable(...)
    loss = photometric_loss(img, target)          # 0-dim, on the image's device
    loss.backward()
"""
import torch
from torch.autograd.function import once_differentiable

WINDOW, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def gaussian_window(dtype=torch.float64, device=None) -> torch.Tensor:
    """The 1-D window g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in float64, then cast."""
    i = torch.arange(WINDOW, dtype=torch.float64) - WINDOW // 2
    g = torch.exp(-i * i / (2 * SIGMA * SIGMA))
    return (g / g.sum()).to(dtype=dtype, device=device)


def _nchw(t):
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4:
        raise ValueError(f"expected an (H, W, C) or (B, H, W, C) image, got shape {tuple(t.shape)}")
    return t.permute(0, 3, 1, 2)


def _pair(img, target):
    if img.shape != target.shape:
        raise ValueError(f"image {tuple(img.shape)} and target {tuple(target.shape)} differ in shape")
    if not img.is_floating_point():
        raise ValueError("images must be floating point")
    return _nchw(img), _nchw(target.to(img.dtype))


def _windowed(t, w2d):
    C = t.shape[1]
    return torch.nn.functional.conv2d(t, w2d.expand(C, 1, WINDOW, WINDOW), padding=WINDOW // 2, groups=C)


def ssim_map_torch(img: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """The per-pixel, per-channel SSIM of two (H, W, C) or (B, H, W, C) images, in the images' own layout."""
    x, y = _pair(img, target)
    g = gaussian_window()
    w2d = (g[:, None] * g[None, :]).to(dtype=x.dtype, device=x.device)
    mu_x, mu_y = _windowed(x, w2d), _windowed(y, w2d)
    s_xx = _windowed(x * x, w2d) - mu_x * mu_x
    s_yy = _windowed(y * y, w2d) - mu_y * mu_y
    s_xy = _windowed(x * y, w2d) - mu_x * mu_y
    m = ((2 * mu_x * mu_y + C1) * (2 * s_xy + C2)) / ((mu_x * mu_x + mu_y * mu_y + C1) * (s_xx + s_yy + C2))
    m = m.permute(0, 2, 3, 1)
    return m[0] if img.dim() == 3 else m


def ssim_torch(img: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Mean SSIM over all pixels, channels and batch entries (0-dim)."""
    return ssim_map_torch(img, target).mean()


def photometric_loss_torch(img: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2, return_parts: bool = False):
    """``(1 - lambda_dssim) * mean|img - target| + lambda_dssim * (1 - ssim)``; d|x - y|/dx is 0 at x == y."""
    _check_lambda(lambda_dssim)
    ssim_v = ssim_torch(img, target)
    l1 = (img - target.to(img.dtype)).abs().mean()
    loss = (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ssim_v)
    return (loss, l1.detach(), ssim_v.detach()) if return_parts else loss


def _check_lambda(lambda_dssim):
    if not 0.0 <= float(lambda_dssim) <= 1.0:
        raise ValueError(f"lambda_dssim must lie in [0, 1], got {lambda_dssim}")


# ------------------------------------------------------------------ backend="hip"
def _hip_forward(x, y, lambda_dssim, keep):
    """x, y: float32 contiguous (B, H, W, C) on one GPU -> (out3 = [loss, l1, ssim], workspace)."""
    from . import _hip
    L = _hip.lib()
    B, H, W, C = x.shape
    nbytes = L.ms_photometric_loss_workspace_bytes(B, H, W, C, int(keep))
    if nbytes == 0:
        # the library's own message (bad C, an image that needs 64-bit offsets ...)
        _hip.check(L.ms_photometric_loss_fwd(B, H, W, C, _hip.ptr(x), _hip.ptr(y), lambda_dssim, None, 0, int(keep),
                                             None, None), "ms_photometric_loss_fwd")
    with _hip.on_device(x.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        out3 = torch.empty(3, dtype=torch.float32, device=x.device)
        _hip.check(L.ms_photometric_loss_fwd(B, H, W, C, _hip.ptr(x), _hip.ptr(y), lambda_dssim, _hip.ptr(ws), nbytes,
                                             int(keep), _hip.ptr(out3), _hip.stream(x.device)), "ms_photometric_loss_fwd")
    return out3, ws


class _PhotometricLossHip(torch.autograd.Function):
    """ms_photometric_loss_fwd / _bwd.  Returns (loss, [l1, ssim]): two views of the device triple, the second one not
    differentiable.  The forward keeps the three derivative maps (in its workspace) only when `keep`."""

    @staticmethod
    def forward(ctx, img, x, y, lambda_dssim, keep):
        out3, ws = _hip_forward(x, y, lambda_dssim, keep)
        ctx.lam, ctx.keep, ctx.img_meta = lambda_dssim, keep, (img.shape, img.dtype)
        if keep:
            # x is img itself when that is float32 and contiguous: nothing of image size is copied or kept twice
            ctx.save_for_backward(x, y, ws)
        parts = out3[1:]
        ctx.mark_non_differentiable(parts)
        return out3[0], parts

    @staticmethod
    @once_differentiable
    def backward(ctx, v_loss, _v_parts):
        from . import _hip
        if not ctx.keep:
            raise RuntimeError("photometric_loss: this forward kept nothing for a backward (img did not require grad)")
        x, y, ws = ctx.saved_tensors
        L = _hip.lib()
        B, H, W, C = x.shape
        with _hip.on_device(x.device):
            v_loss = _hip.f32c(v_loss)
            v_img = torch.empty(ctx.img_meta[0], dtype=torch.float32, device=x.device)   # img's own shape: autograd keeps it as img.grad
            _hip.check(L.ms_photometric_loss_bwd(B, H, W, C, _hip.ptr(x), _hip.ptr(y), ctx.lam, _hip.ptr(ws), ws.numel(),
                                                 _hip.ptr(v_loss), _hip.ptr(v_img), _hip.stream(x.device)),
                       "ms_photometric_loss_bwd")
        return v_img.to(ctx.img_meta[1]), None, None, None, None


def _hip_inputs(img, target):
    from . import _hip
    if isinstance(target, torch.Tensor) and target.requires_grad:
        raise ValueError("backend='hip' differentiates the loss with respect to img only (target is data); "
                         "use backend=\"torch\" for a target that requires grad")
    _hip.require_cuda(img, target, what="image")
    if img.shape != target.shape:
        raise ValueError(f"image {tuple(img.shape)} and target {tuple(target.shape)} differ in shape")
    if img.dim() not in (3, 4) or not img.is_floating_point() or not target.is_floating_point():
        raise ValueError(f"expected floating-point (H, W, C) or (B, H, W, C) images, got shape {tuple(img.shape)}")
    if target.device != img.device:
        raise ValueError(f"target is on {target.device}, the image on {img.device}")
    x, y = _hip.f32c(img.detach()), _hip.f32c(target)
    if x.dim() == 3:
        x, y = x[None], y[None]
    return x, y


def photometric_loss(img: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2, backend: str = "hip",
                     return_parts: bool = False):
    """The 3DGS training loss of a render against its target -> a 0-dim tensor on the image's device.

    img, target: (H, W, C) or (B, H, W, C), C in 1..4 on the HIP path.  ``backend="hip"`` runs the fused kernels
    (csrc/loss.hip): differentiable in ``img`` (once), ``target`` is data; no fallback.  ``backend="torch"`` is the
    definition, ``photometric_loss_torch``.  ``return_parts=True`` returns ``(loss, l1, ssim)``, the last two detached.
    """
    if backend == "torch":
        return photometric_loss_torch(img, target, lambda_dssim, return_parts)
    if backend != "hip":
        raise ValueError("Invalid backend")
    _check_lambda(lambda_dssim)
    x, y = _hip_inputs(img, target)
    keep = bool(img.requires_grad and torch.is_grad_enabled())
    if keep:
        loss, parts = _PhotometricLossHip.apply(img, x, y, float(lambda_dssim), True)
    else:
        out3, _ = _hip_forward(x, y, float(lambda_dssim), False)
        loss, parts = out3[0], out3[1:]
    return (loss, parts[0], parts[1]) if return_parts else loss


def ssim(img: torch.Tensor, target: torch.Tensor, backend: str = "hip") -> torch.Tensor:
    """Mean SSIM (the evaluation metric) -> 0-dim.  On the HIP path: the loss's forward, not differentiable."""
    if backend == "torch":
        return ssim_torch(img, target)
    if backend != "hip":
        raise ValueError("Invalid backend")
    x, y = _hip_inputs(img, target)
    out3, _ = _hip_forward(x, y, 0.2, False)
    return out3[2]


__all__ = ["photometric_loss", "ssim", "photometric_loss_torch", "ssim_torch", "ssim_map_torch", "gaussian_window"]
