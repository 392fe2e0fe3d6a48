"""Bilateral-grid colour correction: a learned, per-image grid of 3x4 colour transforms between the render and the loss.

Photographs of one scene differ in exposure and white balance; a trainer that cannot express that explains it with
floaters and view-dependent colour.  gsplat learns a bilateral grid per image (``use_bilateral_grid``, lib_bilagrid.py),
Kerbl et al.'s code a 3x4 exposure matrix per image -- which is a grid of size 1 x 1 x 1.  ``bilagrid_slice_torch`` and
``bilagrid_tv_loss_torch`` are the definitions, in plain torch with explicit gathers (any device, any float dtype,
differentiated by autograd); ``bilagrid_slice`` / ``bilagrid_tv_loss`` with ``backend="hip"`` are the fused kernels of
csrc/bilagrid.hip::

    grids = bilagrid_identity(len(cameras)); grid_opt = GaussianAdam({"bilagrid": grids}, lr=2e-3)
    img = bilagrid_slice(grids[view], render_gaussians_trainable(...))
    loss = photometric_loss(img, target) + 10.0 * bilagrid_tv_loss(grids)

The slice, for pixel (y, x) of image b with colour (r, g, bl), under a grid of (Gw, Gh, L) vertices:
    u = (x + 0.5) / W * (Gw - 1),  v = (y + 0.5) / H * (Gh - 1),  z = ((r * 0.299 + g * 0.587) + bl * 0.114) * (L - 1);
per axis with coordinate t and size n: index 0 with weight 1 if n == 1, else tc = clamp(t, 0, n - 1),
i0 = min(floor(tc), n - 2), f = tc - i0 and the weights (1 - f, f) on (i0, i0 + 1); A = the 12 coefficients interpolated
over the up to eight vertices (z, v, u); out_i = sum_j A[4 i + j] rgb_j + A[4 i + 3].  Nothing flows into u and v; through
z the gradient is (L - 1) dA/df where 0 < z < L - 1 and zero elsewhere (grid_sample's border rule): a black pixel passes
nothing through the guidance.  This is gsplat's ``grid_sample(grids, (xyz - 0.5) * 2, align_corners=True,
padding_mode="border")`` followed by the 3x4 product.
"""
import torch
from torch.autograd.function import once_differentiable

GRAY = (0.299, 0.587, 0.114)


def bilagrid_identity(num: int, grid=(16, 16, 8), device=None, requires_grad: bool = True) -> torch.Tensor:
    """``num`` identity grids -> (num, 12, L, Gh, Gw) float32, gsplat's ``BilateralGrid.grids`` layout; grid = (Gw, Gh, L).

    Coefficient c = 4 i + j is entry (i, j) of the 3x4 matrix (j = 3: the offset): 0, 5 and 10 are 1, the rest 0."""
    Gw, Gh, L = (int(v) for v in grid)
    if num < 0 or min(Gw, Gh, L) < 1:
        raise ValueError(f"bilagrid_identity: num {num}, grid {tuple(grid)}")
    g = torch.zeros(num, 12, L, Gh, Gw, dtype=torch.float32, device=device)
    g[:, (0, 5, 10)] = 1.0
    return g.requires_grad_(requires_grad)


def _shapes(grids, img):
    """-> (grids as (B, 12, L, Gh, Gw), img as (B, H, W, 3)) or ValueError."""
    if not (isinstance(grids, torch.Tensor) and isinstance(img, torch.Tensor)):
        raise ValueError("bilagrid_slice: grids and img must be tensors")
    if not grids.is_floating_point() or not img.is_floating_point():
        raise ValueError("bilagrid_slice: grids and img must be floating point")
    if (grids.dim(), img.dim()) == (4, 3):
        grids, img = grids[None], img[None]
    elif (grids.dim(), img.dim()) != (5, 4):
        raise ValueError(f"bilagrid_slice: expected grids (B, 12, L, Gh, Gw) with img (B, H, W, 3), or (12, L, Gh, Gw) with "
                         f"(H, W, 3); got {tuple(grids.shape)} and {tuple(img.shape)}")
    if grids.shape[1] != 12 or img.shape[-1] != 3 or grids.shape[0] != img.shape[0]:
        raise ValueError(f"bilagrid_slice: grids {tuple(grids.shape)} (12 coefficients) and img {tuple(img.shape)} (C = 3) "
                         f"do not go together")
    if grids.device != img.device:
        raise ValueError(f"bilagrid_slice: grids are on {grids.device}, the image on {img.device}")
    return grids, img


def _axis(t, n):
    """The definition's axis rule -> [(index, weight), ...]: one pair for n == 1, two otherwise.  The gradient flows into
    t where 0 < t < n - 1 only."""
    if n == 1:
        return [(torch.zeros_like(t, dtype=torch.long), torch.ones_like(t))]
    td = t.detach()
    tc = td.clamp(0, n - 1)
    i0 = tc.floor().clamp(max=n - 2)
    inside = (td > 0) & (td < n - 1)
    f = torch.where(inside, t, tc) - i0
    i0 = i0.long()
    return [(i0, 1 - f), (i0 + 1, f)]


def bilagrid_slice_torch(grids: torch.Tensor, img: torch.Tensor) -> torch.Tensor:
    """The definition of the slice (module docstring): the corrected image, in img's shape and dtype."""
    g, x = _shapes(grids, img)
    B, _, L, Gh, Gw = g.shape
    H, W = x.shape[1:3]
    dt, dev = x.dtype, x.device
    g = g.to(dt).permute(0, 2, 3, 4, 1)                                     # (B, L, Gh, Gw, 12)
    u = (torch.arange(W, dtype=dt, device=dev) + 0.5) / W * (Gw - 1)
    v = (torch.arange(H, dtype=dt, device=dev) + 0.5) / H * (Gh - 1)
    r, gr, bl = x.unbind(-1)
    z = ((r * GRAY[0] + gr * GRAY[1]) + bl * GRAY[2]) * (L - 1)
    bi = torch.arange(B, device=dev)[:, None, None]
    A = None
    for zi, wz in _axis(z, L):
        for yi, wy in _axis(v, Gh):
            for xi, wx in _axis(u, Gw):
                w = (wy[None, :, None] * wx[None, None, :]) * wz
                term = w[..., None] * g[bi, zi, yi[None, :, None], xi[None, None, :]]
                A = term if A is None else A + term
    A = A.reshape(B, H, W, 3, 4)
    out = (A[..., :3] * x[..., None, :]).sum(-1) + A[..., 3]
    return out[0] if img.dim() == 3 else out


def _grids5(grids, who):
    if not isinstance(grids, torch.Tensor) or not grids.is_floating_point():
        raise ValueError(f"{who}: grids must be a floating-point tensor")
    if grids.dim() == 4:
        grids = grids[None]
    if grids.dim() != 5 or grids.shape[1] != 12 or grids.numel() == 0:
        raise ValueError(f"{who}: expected grids (B, 12, L, Gh, Gw) or (12, L, Gh, Gw), got {tuple(grids.shape)}")
    return grids


def bilagrid_tv_loss_torch(grids: torch.Tensor) -> torch.Tensor:
    """gsplat's ``total_variation_loss``: per grid axis of size n >= 2 the mean squared difference of neighbours along it,
    the three added and averaged over the batch (0-dim).  An axis of size 1 contributes 0."""
    g = _grids5(grids, "bilagrid_tv_loss")
    B = g.shape[0]
    total = (g * 0).sum()                  # (zero, and a function of the grids even when no axis has neighbours)
    for dim in (4, 3, 2):
        n = g.shape[dim]
        if n >= 2:
            d = g.narrow(dim, 1, n - 1) - g.narrow(dim, 0, n - 1)
            total = total + (d * d).sum() / (d.numel() // B)
    return total / B


# ------------------------------------------------------------------ backend="hip"
def _dims(g, x):
    B, _, L, Gh, Gw = g.shape
    return B, x.shape[1], x.shape[2], L, Gh, Gw


def _slice_fwd_hip(g, x):
    """g, x: float32 contiguous (B, 12, L, Gh, Gw) and (B, H, W, 3) on one GPU -> out (B, H, W, 3)."""
    from . import _hip
    L = _hip.lib()
    with _hip.on_device(x.device):
        out = torch.empty_like(x)
        _hip.check(L.ms_bilagrid_slice_fwd(*_dims(g, x), _hip.ptr(g), _hip.ptr(x), _hip.ptr(out), _hip.stream(x.device)),
                   "ms_bilagrid_slice_fwd")
    return out


class _BilagridSliceHip(torch.autograd.Function):
    """ms_bilagrid_slice_fwd / _bwd.  g and x are the float32 contiguous forms of grids and img (the tensors themselves
    where they already are): nothing of image size is copied or kept twice."""

    @staticmethod
    def forward(ctx, grids, img, g, x):
        out = _slice_fwd_hip(g, x)
        ctx.meta = (grids.shape, grids.dtype, img.shape, img.dtype)
        ctx.save_for_backward(g, x)
        return out.reshape(img.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, v_out):
        from . import _hip
        g, x = ctx.saved_tensors
        gshape, gdtype, ishape, idtype = ctx.meta
        need_g, need_x = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        L = _hip.lib()
        dims = _dims(g, x)
        with _hip.on_device(x.device):
            v_out = _hip.f32c(v_out)
            v_g = torch.empty(gshape, dtype=torch.float32, device=x.device) if need_g else None
            v_x = torch.empty(ishape, dtype=torch.float32, device=x.device) if need_x else None
            nbytes = L.ms_bilagrid_slice_workspace_bytes(*dims) if need_g else 0
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if need_g else None
            _hip.check(L.ms_bilagrid_slice_bwd(*dims, _hip.ptr(g), _hip.ptr(x), _hip.ptr(v_out), _hip.ptr(ws), nbytes,
                                               _hip.ptr(v_g), _hip.ptr(v_x), _hip.stream(x.device)), "ms_bilagrid_slice_bwd")
        return (v_g.to(gdtype) if need_g else None), (v_x.to(idtype) if need_x else None), None, None


def _f32_on_gpu(who, *tensors):
    from . import _hip
    _hip.require_cuda(*tensors, what="input")
    for t in tensors:
        if t.dtype != torch.float32:
            raise ValueError(f"{who}: backend='hip' takes float32 tensors, got {t.dtype} (backend=\"torch\" takes any float dtype)")


def bilagrid_slice(grids: torch.Tensor, img: torch.Tensor, backend: str = "hip") -> torch.Tensor:
    """Apply bilateral grids to images -> the corrected image in img's shape.

    grids (B, 12, L, Gh, Gw) with img (B, H, W, 3), or (12, L, Gh, Gw) with (H, W, 3); the caller picks the views:
    ``bilagrid_slice(grids[ids], imgs)``.  ``backend="hip"`` runs csrc/bilagrid.hip on float32 tensors of one ROCm device,
    differentiable once in both arguments, no fallback; ``backend="torch"`` is the definition, ``bilagrid_slice_torch``."""
    if backend == "torch":
        return bilagrid_slice_torch(grids, img)
    if backend != "hip":
        raise ValueError("Invalid backend")
    from . import _hip
    g5, x4 = _shapes(grids, img)
    _f32_on_gpu("bilagrid_slice", grids, img)
    g, x = _hip.f32c(g5.detach()), _hip.f32c(x4.detach())
    if torch.is_grad_enabled() and (grids.requires_grad or img.requires_grad):
        return _BilagridSliceHip.apply(grids, img, g, x)
    return _slice_fwd_hip(g, x).reshape(img.shape)


def _tv_fwd_hip(g):
    from . import _hip
    L = _hip.lib()
    B, _, Lz, Gh, Gw = g.shape
    nbytes = L.ms_bilagrid_tv_workspace_bytes(B, Lz, Gh, Gw)
    with _hip.on_device(g.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=g.device) if nbytes else None   # (0: the library's own message)
        out = torch.empty(1, dtype=torch.float32, device=g.device)
        _hip.check(L.ms_bilagrid_tv_fwd(B, Lz, Gh, Gw, _hip.ptr(g), _hip.ptr(ws), nbytes, _hip.ptr(out),
                                        _hip.stream(g.device)), "ms_bilagrid_tv_fwd")
    return out[0]


class _BilagridTvHip(torch.autograd.Function):
    """ms_bilagrid_tv_fwd / _bwd; the backward reads v_loss on the device."""

    @staticmethod
    def forward(ctx, grids, g):
        ctx.meta = (grids.shape, grids.dtype)
        ctx.save_for_backward(g)
        return _tv_fwd_hip(g)

    @staticmethod
    @once_differentiable
    def backward(ctx, v_loss):
        from . import _hip
        (g,) = ctx.saved_tensors
        L = _hip.lib()
        B, _, Lz, Gh, Gw = g.shape
        with _hip.on_device(g.device):
            v_loss = _hip.f32c(v_loss)
            v_g = torch.empty(ctx.meta[0], dtype=torch.float32, device=g.device)
            _hip.check(L.ms_bilagrid_tv_bwd(B, Lz, Gh, Gw, _hip.ptr(g), _hip.ptr(v_loss), _hip.ptr(v_g),
                                            _hip.stream(g.device)), "ms_bilagrid_tv_bwd")
        return v_g.to(ctx.meta[1]), None


def bilagrid_tv_loss(grids: torch.Tensor, backend: str = "hip") -> torch.Tensor:
    """The total-variation regulariser of bilateral grids -> a 0-dim tensor on the grids' device (gsplat weighs it 10).

    ``backend="hip"``: csrc/bilagrid.hip on float32 grids of a ROCm device, differentiable once, no fallback;
    ``backend="torch"`` is the definition, ``bilagrid_tv_loss_torch``."""
    if backend == "torch":
        return bilagrid_tv_loss_torch(grids)
    if backend != "hip":
        raise ValueError("Invalid backend")
    from . import _hip
    g5 = _grids5(grids, "bilagrid_tv_loss")
    _f32_on_gpu("bilagrid_tv_loss", grids)
    g = _hip.f32c(g5.detach())
    if torch.is_grad_enabled() and grids.requires_grad:
        return _BilagridTvHip.apply(grids, g)
    return _tv_fwd_hip(g)


__all__ = ["bilagrid_identity", "bilagrid_slice", "bilagrid_tv_loss", "bilagrid_slice_torch", "bilagrid_tv_loss_torch"]
