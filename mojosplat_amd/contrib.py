"""Per-Gaussian contribution statistics: which Gaussians matter to the images, and which lie under a region of one.

Between training and export two questions come up that neither the renderer nor ``densify_and_prune`` answers.  Pruning for
viewers goes by a Gaussian's blend weight ``w = alpha * T`` over the training views: RadSplat drops what never reaches
``max w >= 0.01`` on any ray, LightGaussian drops the lowest by ``sum w``.  Editors select by painting on a view: a 2D mask
is lifted to the Gaussians whose contribution falls mostly inside it; error-driven densification wants the same sum under a
per-pixel error map.  ``ContributionStats`` holds the four per-Gaussian accumulators, ``accumulate_contributions`` adds one
view to them (``backend="hip"``: ``csrc/contrib.hip``, ``ms_contrib_accumulate``, one launch beside the frame path)::

    stats = ContributionStats(N, device)
    for cam in cameras:
        accumulate_contributions(stats, means3d, scales, quats, opacities, cam)
    keep = select_by_contribution(stats, min_max_weight=0.01)
    params = prune_scene(params, keep, opt)

The definition (``contributions_from_lists_torch``).  Every pixel composites its tile's sorted list front to back with the
package's rules: ``sigma = 0.5 (a dx^2 + c dy^2) + b dx dy`` at the pixel centre, ``alpha = min(0.999, o exp(-sigma))``, an
entry is skipped when ``sigma < 0`` or ``alpha < 1/255``, and the pixel stops before adding an entry when
``T (1 - alpha) <= 1e-4``.  An entry that is added is *blended*, with weight ``w = alpha * T_before``.  Per Gaussian:

  ``pixels``      int64    the number of (view, pixel) pairs in which it was blended
  ``max_weight``  float32  the largest ``w`` over those pairs
  ``sum_q``       int64    ``sum w`` in units of 2^-30: the partial sum of a (view, tile, Gaussian) is rounded to the
                           nearest unit and added as an integer, so accumulation over tiles and views does not depend on
                           their order (2^30 leaves room for 2^31 blended pixels; the step of 9e-10 is far below the
                           smallest single term, (1/255) 1e-4 = 4e-7)
  ``wsum_q``      int64    the same with every term times ``weights[y, x]``, an optional (H, W) map read clamped to [0, 1]
                           with NaN as 0; untouched when no map is given

The HIP kernel rounds the partial of a 16x16 pixel block (at ``tile_size=32`` a tile is four) and sums in float32.
"""
import math

import torch

FIXED_ONE = 1 << 30
ALPHA_THRESHOLD = 1.0 / 255.0
MAX_ALPHA = 0.999
TRANSMITTANCE_STOP = 1e-4

_BUFFERS = (("pixels", torch.int64), ("max_weight", torch.float32), ("sum_q", torch.int64), ("wsum_q", torch.int64))


class ContributionStats:
    """``pixels``, ``max_weight``, ``sum_q``, ``wsum_q``: four contiguous [N] tensors on one device, owned by the caller.
    The methods are plain torch ops that keep the buffers aligned with a changing N, as ``DensifyStats``'s do."""

    def __init__(self, n: int, device=None, *, _buffers=None):
        if _buffers is not None:
            self.pixels, self.max_weight, self.sum_q, self.wsum_q = _buffers
            return
        self.pixels, self.max_weight, self.sum_q, self.wsum_q = (torch.zeros(int(n), dtype=dt, device=device)
                                                                 for _, dt in _BUFFERS)

    def _all(self):
        return self.pixels, self.max_weight, self.sum_q, self.wsum_q

    @property
    def n(self) -> int:
        return self.pixels.numel()

    @property
    def device(self) -> torch.device:
        return self.pixels.device

    def reset(self) -> "ContributionStats":
        for t in self._all():
            t.zero_()
        return self

    def weight_sum(self) -> torch.Tensor:
        """``sum w`` over everything accumulated, float64 [N]."""
        return self.sum_q.to(torch.float64) * (1.0 / FIXED_ONE)

    def weighted_sum(self) -> torch.Tensor:
        """``sum weights * w`` over every call that was given a weight map, float64 [N]."""
        return self.wsum_q.to(torch.float64) * (1.0 / FIXED_ONE)

    def select(self, index_or_mask) -> "ContributionStats":
        """New statistics for the kept (boolean mask) or gathered (index; repeats for clones) Gaussians."""
        return ContributionStats(0, _buffers=tuple(t[index_or_mask].contiguous() for t in self._all()))

    def append(self, n_new: int) -> "ContributionStats":
        """``n_new`` zero entries at the end (Gaussians added behind the existing ones); in place."""
        self.pixels, self.max_weight, self.sum_q, self.wsum_q = (
            torch.cat([t, torch.zeros(int(n_new), dtype=t.dtype, device=t.device)]) for t in self._all())
        return self

    def check(self, n: int, device: torch.device):
        """ValueError unless the buffers fit a view of ``n`` Gaussians on ``device`` (what the HIP kernel writes)."""
        for name, dt in _BUFFERS:
            t = getattr(self, name)
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != n:
                raise ValueError(f"stats.{name}: expected a tensor of shape [{n}] (one entry per Gaussian), "
                                 f"got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            if t.dtype != dt:
                raise ValueError(f"stats.{name}: expected {dt}, got {t.dtype}")
            if t.device != device:
                raise ValueError(f"stats.{name} is on {t.device}, the Gaussians on {device}")
            if not t.is_contiguous():
                raise ValueError(f"stats.{name} must be contiguous")


# ---------------------------------------------------------------------------------------------------------------------------
# checks (all of them before anything is launched)

def _check_backend(backend):
    if backend not in ("hip", "torch"):
        raise ValueError(f"Invalid backend: {backend}")


def _check_tile_size(tile_size):
    if tile_size not in (16, 32):
        raise ValueError(f"tile_size must be 16 or 32, got {tile_size!r}")


def _check_camera(camera):
    from .utils import Camera
    if not isinstance(camera, Camera):
        raise ValueError(f"camera must be a Camera, got {type(camera).__name__}")
    if not (isinstance(camera.H, int) and isinstance(camera.W, int) and camera.H > 0 and camera.W > 0):
        raise ValueError(f"camera: H and W must be positive integers, got H = {camera.H!r}, W = {camera.W!r}")


def _check_weights(weights, camera, device):
    if weights is None:
        return
    if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (camera.H, camera.W):
        raise ValueError(f"weights: expected a tensor of shape {(camera.H, camera.W)} (H, W), got "
                         f"{tuple(weights.shape) if isinstance(weights, torch.Tensor) else type(weights).__name__}")
    if not (weights.dtype.is_floating_point or weights.dtype in (torch.bool, torch.uint8)):
        raise ValueError(f"weights: expected a floating-point, bool or uint8 map, got {weights.dtype}")
    if weights.device != device:
        raise ValueError(f"weights is on {weights.device}, the Gaussians on {device}")


def _check_lists(stats, means2d, conics, opacities, tile_ranges, sorted_ids, camera, weights, tile_size, backend):
    _check_backend(backend)
    _check_tile_size(tile_size)
    _check_camera(camera)
    if not isinstance(stats, ContributionStats):
        raise ValueError(f"stats must be a ContributionStats, got {type(stats).__name__}")
    for name, t in (("means2d", means2d), ("conics", conics), ("opacities", opacities), ("tile_ranges", tile_ranges),
                    ("sorted_ids", sorted_ids)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if means2d.dim() != 2 or means2d.shape[1] != 2 or not means2d.dtype.is_floating_point:
        raise ValueError(f"means2d: expected a floating-point tensor of shape (N, 2), got {tuple(means2d.shape)} {means2d.dtype}")
    N, dev = means2d.shape[0], means2d.device
    if tuple(conics.shape) != (N, 3) or not conics.dtype.is_floating_point:
        raise ValueError(f"conics: expected a floating-point tensor of shape {(N, 3)}, got {tuple(conics.shape)} {conics.dtype}")
    if tuple(opacities.shape) not in ((N,), (N, 1)) or not opacities.dtype.is_floating_point:
        raise ValueError(f"opacities: expected a floating-point tensor of shape {(N,)} or {(N, 1)}, got "
                         f"{tuple(opacities.shape)} {opacities.dtype}")
    th, tw = -(-camera.H // tile_size), -(-camera.W // tile_size)
    if tuple(tile_ranges.shape) != (th, tw, 2) or tile_ranges.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"tile_ranges: expected an int32 or int64 tensor of shape {(th, tw, 2)}, got "
                         f"{tuple(tile_ranges.shape)} {tile_ranges.dtype}")
    if sorted_ids.dim() != 1 or sorted_ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"sorted_ids: expected a 1-D int32 or int64 tensor, got {tuple(sorted_ids.shape)} {sorted_ids.dtype}")
    for name, t in (("conics", conics), ("opacities", opacities), ("tile_ranges", tile_ranges), ("sorted_ids", sorted_ids)):
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, means2d on {dev}")
    _check_weights(weights, camera, dev)
    stats.check(N, dev)
    if backend == "hip":
        from . import _hip
        _hip.require_cuda(means2d, what="list")
        _hip.lib()
    return N, dev, th, tw


def _clamped_weights(weights, dtype):
    """The map as both backends read it: [0, 1], NaN as 0."""
    w = weights.to(torch.float32)
    return torch.nan_to_num(w, nan=0.0, posinf=1.0, neginf=0.0).clamp(0.0, 1.0).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# the definition

@torch.no_grad()
def contributions_from_lists_torch(stats, means2d, conics, opacities, tile_ranges, sorted_ids, camera, *, weights=None,
                                   tile_size=16, _probe=None):
    """The definition, in the dtype of ``means2d`` (float64 lists give the float64 reference), tile by tile, on any device.
    ``_probe(ty, tx, ids, xs, ys, alpha, valid, live, t_before, t_after)`` is called per non-empty tile with the
    (entries, pixels) arrays of the walk (tests mark near-threshold pairs with it)."""
    N, dev, th, tw = _check_lists(stats, means2d, conics, opacities, tile_ranges, sorted_ids, camera, weights, tile_size, "torch")
    dt = means2d.dtype
    H, W, ts = camera.H, camera.W, tile_size
    conics, op = conics.to(dt), opacities.reshape(-1).to(dt)
    wmap = None if weights is None else _clamped_weights(weights, dt)
    ids_all = sorted_ids.long()
    M = ids_all.numel()
    ranges = tile_ranges.tolist()
    for ty in range(th):
        for tx in range(tw):
            s, e = ranges[ty][tx]
            s, e = max(s, 0), min(e, M)
            if e <= s:
                continue
            y0, x0 = ty * ts, tx * ts
            y1, x1 = min(y0 + ts, H), min(x0 + ts, W)
            py, px = torch.meshgrid(torch.arange(y0, y1, dtype=dt, device=dev) + 0.5,
                                    torch.arange(x0, x1, dtype=dt, device=dev) + 0.5, indexing="ij")
            px, py = px.reshape(1, -1), py.reshape(1, -1)
            g = ids_all[s:e]
            dx = means2d[g, 0][:, None] - px
            dy = means2d[g, 1][:, None] - py
            ca, cb, cc = conics[g, 0][:, None], conics[g, 1][:, None], conics[g, 2][:, None]
            sigma = 0.5 * (ca * dx * dx + cc * dy * dy) + cb * dx * dy
            alpha = torch.clamp(op[g][:, None] * torch.exp(-sigma), max=MAX_ALPHA)
            valid = (sigma >= 0) & (alpha >= ALPHA_THRESHOLD)
            a = torch.where(valid, alpha, torch.zeros_like(alpha))
            t_after = torch.cumprod(1 - a, dim=0)
            live = valid & (t_after > TRANSMITTANCE_STOP)        # prefix-closed: t_after only falls
            a = torch.where(live, a, torch.zeros_like(a))
            t_after = torch.cumprod(1 - a, dim=0)                 # the transmittance behind each entry of the live prefix
            t_before = torch.cat([torch.ones_like(t_after[:1]), t_after[:-1]], 0)
            w = a * t_before
            if _probe is not None:
                _probe(ty, tx, g, px.reshape(-1), py.reshape(-1), alpha, valid, live, t_before, t_after)
            stats.pixels.index_add_(0, g, live.sum(1))
            stats.max_weight.scatter_reduce_(0, g, w.max(1).values.to(torch.float32), "amax", include_self=True)
            stats.sum_q.index_add_(0, g, torch.round(w.sum(1) * FIXED_ONE).to(torch.int64))
            if wmap is not None:
                wt = wmap[y0:y1, x0:x1].reshape(1, -1)
                stats.wsum_q.index_add_(0, g, torch.round((w * wt).sum(1) * FIXED_ONE).to(torch.int64))
    return stats


# ---------------------------------------------------------------------------------------------------------------------------
# the launch

def _contributions_from_lists_hip(stats, N, means2d, conics, opacities, tile_ranges, sorted_ids, camera, weights, tile_size):
    from . import _hip
    L = _hip.lib()
    dev = means2d.device
    ids = sorted_ids.to(torch.int32).contiguous()
    M = ids.numel()
    if N == 0 or M == 0:
        return stats
    means2d, conics, op = _hip.f32c(means2d), _hip.f32c(conics), _hip.f32c(opacities.reshape(-1))
    ranges = tile_ranges.to(torch.int32).contiguous()
    w = None if weights is None else _hip.f32c(weights)
    with _hip.on_device(dev):
        _hip.check(L.ms_contrib_accumulate(N, M, _hip.ptr(means2d), _hip.ptr(conics), _hip.ptr(op), _hip.ptr(ranges), _hip.ptr(ids),
                                           _hip.ptr(w), camera.W, camera.H, tile_size, _hip.ptr(stats.pixels),
                                           _hip.ptr(stats.max_weight), _hip.ptr(stats.sum_q),
                                           None if w is None else _hip.ptr(stats.wsum_q), _hip.stream(dev)),
                   "ms_contrib_accumulate")
    _hip.bump(stats.pixels, stats.max_weight, stats.sum_q, *(() if w is None else (stats.wsum_q,)))
    return stats


def contributions_from_lists(stats, means2d, conics, opacities, tile_ranges, sorted_ids, camera, *, weights=None, tile_size=16,
                             backend="hip") -> ContributionStats:
    """One view added to ``stats`` from the per-stage lists of ``project_gaussians`` and ``bin_gaussians_to_tiles``:
    ``means2d`` (N, 2), ``conics`` (N, 3), activated ``opacities`` (N,), ``tile_ranges`` (th, tw, 2) and the sorted Gaussian
    ids (M,), binned at ``tile_size`` (16 or 32).  ``weights``: None or an (H, W) map, read clamped to [0, 1] with NaN as 0;
    without one ``stats.wsum_q`` is left untouched.  backend="hip": ``ms_contrib_accumulate``, one launch on the current
    stream, no host wait, bitwise reproducible; CUDA/ROCm tensors (float32 inside); no fallback.  backend="torch": the
    definition, in the lists' dtype, on any device.  Every check is made before anything is launched."""
    N, *_ = _check_lists(stats, means2d, conics, opacities, tile_ranges, sorted_ids, camera, weights, tile_size, backend)
    if backend == "torch":
        return contributions_from_lists_torch(stats, means2d, conics, opacities, tile_ranges, sorted_ids, camera,
                                              weights=weights, tile_size=tile_size)
    return _contributions_from_lists_hip(stats, N, means2d, conics, opacities, tile_ranges, sorted_ids, camera, weights, tile_size)


def _check_scene(means3d, scales, quats, opacities, backend):
    _check_backend(backend)
    for name, t in (("means3d", means3d), ("scales", scales), ("quats", quats), ("opacities", opacities)):
        if not isinstance(t, torch.Tensor) or not t.dtype.is_floating_point:
            raise ValueError(f"{name} must be a floating-point tensor, got "
                             f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
    if means3d.dim() != 2 or means3d.shape[1] != 3:
        raise ValueError(f"means3d: expected shape (N, 3), got {tuple(means3d.shape)}")
    N, dev = means3d.shape[0], means3d.device
    for name, t, shapes in (("scales", scales, ((N, 3),)), ("quats", quats, ((N, 4),)), ("opacities", opacities, ((N,), (N, 1)))):
        if tuple(t.shape) not in shapes:
            raise ValueError(f"{name}: expected shape {' or '.join(str(s) for s in shapes)}, got {tuple(t.shape)}")
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, means3d on {dev}")
    if backend == "hip":
        from . import _hip
        _hip.require_cuda(means3d, what="gaussian tensor")
        _hip.lib()
    return N, dev


@torch.no_grad()
def accumulate_contributions(stats, means3d, scales, quats, opacities, camera, *, weights=None, tile_size=16,
                             backend="hip") -> ContributionStats:
    """Project, bin and ``contributions_from_lists`` with the chosen backend's own per-stage functions (log-space
    ``scales``, activated ``opacities``, as ``project_gaussians`` takes them).  backend="torch" runs on CPU tensors too."""
    from .binning import bin_gaussians_to_tiles_hip, bin_gaussians_to_tiles_torch
    from .projection import project_gaussians_hip, project_gaussians_torch
    _check_camera(camera)
    N, dev = _check_scene(means3d, scales, quats, opacities, backend)
    _check_tile_size(tile_size)
    _check_weights(weights, camera, dev)
    if not isinstance(stats, ContributionStats):
        raise ValueError(f"stats must be a ContributionStats, got {type(stats).__name__}")
    stats.check(N, dev)
    th, tw = -(-camera.H // tile_size), -(-camera.W // tile_size)
    project, bins = (project_gaussians_hip, bin_gaussians_to_tiles_hip) if backend == "hip" else \
        (project_gaussians_torch, bin_gaussians_to_tiles_torch)
    means2d, conics, depths, radii = project(means3d.detach(), scales.detach(), quats.detach(), opacities.detach(), camera)
    ids, ranges = bins(means2d, radii, depths, tile_size, tw, th)
    return contributions_from_lists(stats, means2d, conics, opacities.detach(), ranges, ids, camera, weights=weights,
                                    tile_size=tile_size, backend=backend)


# ---------------------------------------------------------------------------------------------------------------------------
# what the statistics are for (torch ops; they run on CPU tensors too)

@torch.no_grad()
def select_by_contribution(stats, *, min_max_weight=None, keep_fraction=None) -> torch.Tensor:
    """-> keep mask, bool [N].  ``min_max_weight=tau``: keep where ``max_weight >= tau`` (RadSplat's rule).
    ``keep_fraction=f``: the ``ceil(f N)`` largest by ``sum_q`` (LightGaussian's score without the volume term), where a
    float64 product ``f N`` within four units in its last place above an integer counts as that integer; ties go to the lower row, a Gaussian that was never blended (``pixels == 0``) ranks behind every one that was.  Both given: the AND
    of the two.  Neither given: ValueError."""
    if not isinstance(stats, ContributionStats):
        raise ValueError(f"stats must be a ContributionStats, got {type(stats).__name__}")
    if min_max_weight is None and keep_fraction is None:
        raise ValueError("give min_max_weight, keep_fraction or both")
    if min_max_weight is not None and not float(min_max_weight) >= 0.0:
        raise ValueError(f"min_max_weight must be >= 0, got {min_max_weight!r}")
    if keep_fraction is not None and not 0.0 <= float(keep_fraction) <= 1.0:
        raise ValueError(f"keep_fraction must lie in [0, 1], got {keep_fraction!r}")
    stats.check(stats.n, stats.device)
    N = stats.n
    keep = torch.ones(N, dtype=torch.bool, device=stats.device)
    if min_max_weight is not None:
        keep &= stats.max_weight >= float(min_max_weight)
    if keep_fraction is not None:
        x = float(keep_fraction) * N
        k = min(N, max(0, math.ceil(x - 4.0 * math.ulp(x))))         # (0.3 * 10 is 3.0000000000000004 in binary)
        key = torch.where(stats.pixels > 0, stats.sum_q, torch.full_like(stats.sum_q, -1))
        order = torch.argsort(key, descending=True, stable=True)
        top = torch.zeros(N, dtype=torch.bool, device=stats.device)
        top[order[:k]] = True
        keep &= top
    return keep


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


@torch.no_grad()
def lift_mask(means3d, scales, quats, opacities, cameras, masks, *, threshold=0.5, tile_size=16, backend="hip"):
    """A 2D mask lifted to the Gaussians under it -> ``(selected bool [N], ratio float64 [N])``.  ``cameras`` and ``masks``:
    one view or equally long sequences; a mask is an (H, W) map of its camera's size (bool, or weights in [0, 1]).
    ``ratio = weighted_sum / weight_sum`` over all views given: the share of a Gaussian's blend weight that falls inside the
    masks (0 where it was never blended); ``selected = ratio > threshold``."""
    cams, maps = _as_list(cameras), _as_list(masks)
    if len(cams) != len(maps) or not cams:
        raise ValueError(f"cameras and masks must be one view or equally long sequences, got {len(cams)} and {len(maps)}")
    if not 0.0 <= float(threshold) <= 1.0:
        raise ValueError(f"threshold must lie in [0, 1], got {threshold!r}")
    for cam in cams:
        _check_camera(cam)
    N, dev = _check_scene(means3d, scales, quats, opacities, backend)
    _check_tile_size(tile_size)
    for cam, m in zip(cams, maps):
        if m is None:
            raise ValueError("lift_mask: every view needs a mask")
        _check_weights(m, cam, dev)
    stats = ContributionStats(N, dev)
    for cam, m in zip(cams, maps):
        accumulate_contributions(stats, means3d, scales, quats, opacities, cam, weights=m.to(torch.float32),
                                 tile_size=tile_size, backend=backend)
    total, inside = stats.weight_sum(), stats.weighted_sum()
    ratio = torch.where(stats.sum_q > 0, inside / total.clamp_min(1.0 / FIXED_ONE), torch.zeros_like(total))
    return ratio > float(threshold), ratio


@torch.no_grad()
def prune_scene(params, keep, opt=None, *, requires_grad=False) -> dict:
    """Every named tensor's rows by the boolean mask ``keep`` [N] -> a dict of new contiguous leaf tensors, order kept.  An
    attached ``GaussianAdam`` follows through ``opt.relocate(new_params, keep, 0)``: the moments keep their rows, ``step``
    is kept."""
    if not isinstance(params, dict) or not params:
        raise ValueError("params must be a non-empty dict {name: tensor}")
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or keep.dim() != 1:
        raise ValueError(f"keep must be a 1-D boolean mask, got "
                         f"{(tuple(keep.shape), keep.dtype) if isinstance(keep, torch.Tensor) else type(keep).__name__}")
    N = keep.numel()
    for name, t in params.items():
        if not isinstance(t, torch.Tensor) or t.dim() == 0 or t.shape[0] != N:
            raise ValueError(f"{name}: expected a tensor of {N} rows (the mask's length), got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.device != keep.device:
            raise ValueError(f"{name} is on {t.device}, keep on {keep.device}")
    new = {name: t.detach()[keep].contiguous().requires_grad_(bool(requires_grad) and t.dtype.is_floating_point)
           for name, t in params.items()}
    if opt is not None:
        opt.relocate(new, keep, 0)
    return new


__all__ = ["ContributionStats", "contributions_from_lists", "contributions_from_lists_torch", "accumulate_contributions",
           "select_by_contribution", "lift_mask", "prune_scene", "FIXED_ONE"]
