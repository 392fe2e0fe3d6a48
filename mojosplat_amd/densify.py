"""Densification statistics of 3D Gaussian Splatting training (adaptive density control).

Kerbl et al.'s training and gsplat's default strategy clone, split and prune Gaussians from three
per-Gaussian sums over the views a Gaussian was visible in: the screen-space positional gradient,
the number of those views and the largest screen radius it reached.  ``DensifyStats`` holds them;
``render_gaussians_trainable(..., densify=stats)`` updates them inside its backward (on the fused
frame: the backward projection's kernel, ``ms_render_bwd_finish_densify``).  ``update_torch`` is the
definition, in plain torch::

    stats = DensifyStats(N, device)
    img = render_gaussians_trainable(..., densify=stats); loss(img).backward()
    grow = stats.mean_grad() > threshold          # then clone / split / prune, and
    stats = stats.select(kept).append(n_new)      # keep the statistics in step with N
"""
import torch


class DensifyStats:
    """``grad2d``, ``count`` and ``max_radii``: float32 [N] on one device, owned by the caller.  The
    methods are plain torch ops that keep the three buffers aligned with a changing N."""

    def __init__(self, n: int, device=None, *, _buffers=None):
        if _buffers is not None:
            self.grad2d, self.count, self.max_radii = _buffers
            return
        z = lambda: torch.zeros(int(n), dtype=torch.float32, device=device)
        self.grad2d, self.count, self.max_radii = z(), z(), z()

    @property
    def n(self) -> int:
        return self.grad2d.numel()

    @property
    def device(self) -> torch.device:
        return self.grad2d.device

    def reset(self) -> "DensifyStats":
        for t in (self.grad2d, self.count, self.max_radii):
            t.zero_()
        return self

    def mean_grad(self) -> torch.Tensor:
        """The mean screen-space gradient over the views a Gaussian was visible in (0 where it never was)."""
        return self.grad2d / self.count.clamp_min(1)

    def select(self, index_or_mask) -> "DensifyStats":
        """New statistics for the kept (boolean mask) or gathered (index; repeats for clones) Gaussians."""
        return DensifyStats(0, _buffers=tuple(t[index_or_mask].contiguous()
                                              for t in (self.grad2d, self.count, self.max_radii)))

    def append(self, n_new: int) -> "DensifyStats":
        """``n_new`` zero entries at the end (Gaussians added behind the existing ones); in place."""
        z = torch.zeros(int(n_new), dtype=torch.float32, device=self.device)
        self.grad2d, self.count, self.max_radii = (torch.cat([t, z]) for t in (self.grad2d, self.count, self.max_radii))
        return self

    def check(self, n: int, device: torch.device):
        """ValueError unless the buffers fit a frame of ``n`` Gaussians on ``device`` (what the HIP update writes)."""
        for name in ("grad2d", "count", "max_radii"):
            t = getattr(self, name)
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != n:
                raise ValueError(f"densify.{name}: expected a tensor of shape [{n}] (one entry per Gaussian), "
                                 f"got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            if t.dtype != torch.float32:
                raise ValueError(f"densify.{name}: expected float32, got {t.dtype}")
            if t.device != device:
                raise ValueError(f"densify.{name} is on {t.device}, the Gaussians on {device}")
            if not t.is_contiguous():
                raise ValueError(f"densify.{name} must be contiguous")


def update_torch(stats: DensifyStats, v_means2d: torch.Tensor, radii: torch.Tensor, W: int, H: int) -> DensifyStats:
    """One view's update, the definition (and the CPU reference of the HIP kernels).  For every
    Gaussian alive in the view (``radii > 0`` in both axes), with g = dL/dmeans2d in pixels:
    ``count += 1``, ``grad2d += |(g_x W / 2, g_y H / 2)|`` (the gradient in NDC units) and
    ``max_radii = max(max_radii, max(r_x, r_y) / max(W, H))``.  Others are left untouched."""
    alive = (radii > 0).all(-1)
    g = v_means2d.to(torch.float32)
    norm = torch.sqrt((g[:, 0] * W / 2) ** 2 + (g[:, 1] * H / 2) ** 2)
    r = radii.max(-1).values.to(torch.float32)
    r = r / torch.full_like(r, max(W, H))   # (elementwise: a scalar divisor becomes a reciprocal product on the GPU)
    stats.grad2d[alive] += norm[alive]
    stats.count[alive] += 1
    stats.max_radii[alive] = torch.maximum(stats.max_radii[alive], r[alive])
    return stats


__all__ = ["DensifyStats", "update_torch"]
