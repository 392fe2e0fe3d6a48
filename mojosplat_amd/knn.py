"""Start a scene from a point cloud: exact k nearest neighbours, the initial parameters, the scene's extent.

Every 3DGS trainer begins from an SfM point cloud (3DGS ``create_from_pcd``, gsplat's ``simple_trainer``) and sets each
Gaussian's initial log-scale from the mean squared distance to its three nearest neighbours -- ``distCUDA2`` of the CUDA
stack's ``simple-knn``::

    params = init_from_points(points, colors, sh_degree=3)          # the dict GaussianAdam, densify_and_prune, grow take
    opt = GaussianAdam(params, lr=...)
    extent = scene_extent(cameras)                                  # densify_and_prune(scene_scale=extent)

``knn_torch`` is the definition (plain torch, any device, chunked over the query rows so that it fits in memory: N^2 work);
``backend="hip"`` runs csrc/knn.hip (``ms_knn``), an exact search over bounding boxes of a Morton order, and is held to the
definition bit for bit -- distances AND indices.

THE DEFINITION.  ``points`` is (N, 3).  For query ``i`` and candidate ``j != i``, in float32 with every operation rounded on
its own (no contraction)::

    dx = x_i - x_j    (dy, dz likewise)        d_ij = ((dx*dx) + (dy*dy)) + (dz*dz)

Self is excluded by ROW, not by distance: duplicate points are each other's neighbours at distance 0.  The candidates are
ordered lexicographically by ``(d_ij, j)`` and the first k are the result, so ``dist2`` (N, k) float32, ascending, and ``idx``
(N, k) int64 are both uniquely defined; they are in the caller's row order.

Checks, all before any launch, each a ValueError: ``1 <= k <= 8``; shape (N, 3); ``k + 1 <= N < 2**31``; for backend="hip"
a CUDA/ROCm, float32, contiguous tensor (no fallback); every coordinate finite.  THE FINITE CHECK COSTS ONE HOST WAIT per
call: this is a once-per-scene call.  The kernel itself makes none.  Squares that overflow float32 are the caller's problem:
the documented range is |coordinate| <= 1e18.

``init_from_points`` returns float32, contiguous leaf tensors::

    means3d   (N, 3)  a copy of points
    scales    (N, 3)  every column log(sqrt(max(m, min_dist2)) * init_scale),
                      m = (((d_0 + d_1) + ...) + d_{k-1}) / float32(k) over knn's dist2 (k = 3 and the defaults: 3DGS's)
    quats     (N, 4)  (1, 0, 0, 0), wxyz
    opacities (N,)    logit(init_opacity) (opacity_space="logit") or init_opacity ("linear")
    features  (N, 3) the colours (sh_degree=None), or (N, (d+1)^2, 3) with [:, 0] = (rgb - 0.5) / 0.2820947917738781 and the
              rest zero (sh_degree=d): evaluate_sh at degree 0 returns the colour

``colors``: (N, 3) float in [0, 1], or uint8 (divided by 255); None means 0.5.  Everything after ``knn`` is the same torch
ops for both backends: the two return bit-identical dicts.

Not covered: k > 8, dimensions other than 3, float16 / float64 points on the HIP path, returning the scene in Morton order
(``prepare_scene`` does that), random initial rotations, the sharded trainer, graph capture.
"""
import math

import torch

from .scene_order import morton_permutation

MAX_K = 8
SH_C0 = 0.2820947917738781
_CHUNK_ELEMENTS = 1 << 24          # distances per chunk of the definition (64 MB in float32, as much again per temporary)


def _validate(points, k, backend):
    if backend not in ("hip", "torch"):
        raise ValueError(f"Invalid backend: {backend!r} (\"hip\" or \"torch\")")
    if not (isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= MAX_K):
        raise ValueError(f"k must be an int in [1, {MAX_K}], got {k!r}")
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or not points.is_floating_point():
        raise ValueError(f"points must be a floating-point tensor of shape (N, 3), got "
                         f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
    N = points.shape[0]
    if not (k + 1 <= N < 2 ** 31):
        raise ValueError(f"points has {N} rows: k + 1 = {k + 1} <= N < 2**31 is required")
    if backend == "hip":
        if not points.is_cuda:
            raise ValueError("backend='hip': points must be a CUDA/ROCm tensor (there is no fallback)")
        if points.dtype != torch.float32:
            raise ValueError(f"backend='hip': points must be float32, got {points.dtype}")
        if not points.is_contiguous():
            raise ValueError("backend='hip': points must be contiguous")
    if not bool(torch.isfinite(points.detach()).all()):          # (the one host wait of a call)
        raise ValueError("points holds a coordinate that is not finite")
    return N


@torch.no_grad()
def knn_torch(points, k=3, *, return_index=True, chunk=None):
    """THE DEFINITION (module docstring), on inputs ``_validate`` has passed -> (dist2 (N, k) float32, idx (N, k) int64 or
    None).  ``chunk`` query rows at a time (None: as many as keep a chunk's distances at 2^24 elements); every chunk size
    gives the same bits."""
    p = points.detach().float()
    N = p.shape[0]
    if chunk is None:
        chunk = max(1, _CHUNK_ELEMENTS // N)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    dist2 = torch.empty((N, k), dtype=torch.float32, device=p.device)
    idx = torch.empty((N, k), dtype=torch.int64, device=p.device) if return_index else None
    for a in range(0, N, chunk):
        b = min(a + chunk, N)
        dx = x[a:b, None] - x[None, :]
        dy = y[a:b, None] - y[None, :]
        dz = z[a:b, None] - z[None, :]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        d = (xx + yy) + zz
        rows = torch.arange(b - a, device=p.device)
        d[rows, rows + a] = float("inf")                         # self, by row
        val, ind = torch.sort(d, dim=1, stable=True)             # ascending in (d, j)
        dist2[a:b] = val[:, :k]
        if return_index:
            idx[a:b] = ind[:, :k]
    return dist2, idx


@torch.no_grad()
def _knn_hip(points, N, k, return_index, order="morton"):
    from . import _hip
    L = _hip.lib()
    dev = points.device
    p = points.detach()
    if isinstance(order, str):
        order = morton_permutation(p).to(torch.int32)            # torch ops on the device, once
    dist2 = torch.empty((N, k), dtype=torch.float32, device=dev)
    idx = torch.empty((N, k), dtype=torch.int64, device=dev) if return_index else None
    with _hip.on_device(dev):
        ws = torch.empty(L.ms_knn_workspace_bytes(N, k), dtype=torch.uint8, device=dev)
        _hip.check(L.ms_knn(N, _hip.ptr(p), _hip.ptr(order), k, _hip.ptr(dist2), _hip.ptr(idx), _hip.ptr(ws), _hip.stream(dev)),
                   "ms_knn")
    return dist2, idx


def knn(points, k=3, *, return_index=True, backend="hip"):
    """The k nearest OTHER rows of every row of ``points`` (N, 3) -> (dist2 (N, k) float32 squared distances, ascending;
    idx (N, k) int64 row numbers, or None with return_index=False), in the caller's row order, ties broken by row number
    (module docstring).  backend="torch": the definition, any device and float dtype (computed in float32), N^2 work.
    backend="hip": ms_knn over the Morton order of the points; CUDA/ROCm, float32, contiguous; bit-identical to the definition;
    no fallback.  One host wait per call (the finite check)."""
    N = _validate(points, k, backend)
    if backend == "torch":
        return knn_torch(points, k, return_index=return_index)
    return _knn_hip(points, N, k, return_index)


def _positive(name, v):
    if not (isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v > 0.0):
        raise ValueError(f"{name} must be a positive finite number, got {v!r}")


def _colors(colors, N, dev):
    """-> (N, 3) float32 in [0, 1] on ``dev``."""
    if colors is None:
        return torch.full((N, 3), 0.5, dtype=torch.float32, device=dev)
    if not isinstance(colors, torch.Tensor) or tuple(colors.shape) != (N, 3):
        raise ValueError(f"colors must be a tensor of shape ({N}, 3) or None")
    if colors.device != dev:
        raise ValueError(f"colors is on {colors.device}, points on {dev}")
    if colors.dtype == torch.uint8:
        return colors.float() / 255.0
    if not colors.is_floating_point():
        raise ValueError(f"colors must be floating point in [0, 1] or uint8, got {colors.dtype}")
    return colors.detach().float().clone()


def init_from_points(points, colors=None, *, sh_degree=None, k=3, init_scale=1.0, init_opacity=0.1, opacity_space="logit",
                     min_dist2=1e-7, requires_grad=True, backend="hip"):
    """The parameters of a scene that starts from the point cloud ``points`` (N, 3), as 3DGS initialises them (module
    docstring): the ``params`` dict that GaussianAdam, densify_and_prune, relocate_dead and grow take -- "means3d", "scales"
    (log space, isotropic, from the mean squared distance to the k nearest neighbours), "quats", "opacities", "features".
    float32, contiguous leaf tensors with ``requires_grad`` as given.  backend: the ``knn`` call's; both give the same bits.
    One host wait (``knn``'s finite check)."""
    from .sh import MAX_SH_DEGREE
    if opacity_space not in ("linear", "logit"):
        raise ValueError(f"Invalid opacity_space: {opacity_space!r} (\"linear\" or \"logit\")")
    if sh_degree is not None and not (isinstance(sh_degree, int) and not isinstance(sh_degree, bool) and 0 <= sh_degree <= MAX_SH_DEGREE):
        raise ValueError(f"sh_degree must be None or an int in [0, {MAX_SH_DEGREE}], got {sh_degree!r}")
    _positive("init_scale", init_scale)
    _positive("min_dist2", min_dist2)
    if not (isinstance(init_opacity, (int, float)) and not isinstance(init_opacity, bool) and 0.0 < init_opacity < 1.0):
        raise ValueError(f"init_opacity must lie in (0, 1), got {init_opacity!r}")
    N = _validate(points, k, backend)
    dev = points.device
    rgb = _colors(colors, N, dev)
    dist2, _ = knn_torch(points, k, return_index=False) if backend == "torch" else _knn_hip(points, N, k, False)
    m = dist2[:, 0]
    for i in range(1, k):
        m = m + dist2[:, i]
    m = m / torch.tensor(float(k), dtype=torch.float32, device=dev)
    log_scale = torch.log(torch.sqrt(torch.clamp_min(m, min_dist2)) * init_scale)
    quats = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    quats[:, 0] = 1.0
    opacity = math.log(init_opacity / (1.0 - init_opacity)) if opacity_space == "logit" else init_opacity
    if sh_degree is None:
        features = rgb
    else:
        features = torch.zeros((N, (sh_degree + 1) ** 2, 3), dtype=torch.float32, device=dev)
        features[:, 0] = (rgb - 0.5) / SH_C0
    params = {"means3d": points.detach().float().clone(),
              "scales": log_scale.unsqueeze(-1).repeat(1, 3),
              "quats": quats,
              "opacities": torch.full((N,), opacity, dtype=torch.float32, device=dev),
              "features": features}
    return {n: t.contiguous().requires_grad_(bool(requires_grad)) for n, t in params.items()}


def scene_extent(cameras) -> float:
    """1.1 x the largest distance of a camera centre (``sh.camera_position``) from the centres' mean: 3DGS's
    ``cameras_extent``, the value ``densify_and_prune(scene_scale=)`` wants.  cameras: a non-empty sequence of Camera.  One
    host wait (the value is a Python float)."""
    from .sh import camera_position
    cameras = list(cameras)
    if not cameras:
        raise ValueError("scene_extent needs at least one camera")
    centres = torch.stack([camera_position(c).detach().double().cpu() for c in cameras])
    return 1.1 * float((centres - centres.mean(0, keepdim=True)).norm(dim=-1).max())


__all__ = ["knn", "knn_torch", "init_from_points", "scene_extent", "MAX_K"]
