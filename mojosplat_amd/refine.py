"""The densification step of 3D Gaussian Splatting training (adaptive density control): clone, split and prune.

Kerbl et al.'s training and gsplat's default strategy grow a scene where the screen-space gradient is high -- a small
Gaussian is cloned, a large one is split in two -- and remove Gaussians that are transparent or too big.
``densify_and_prune`` does all three in ONE pass over the scene, from the statistics a ``DensifyStats`` gathered, and
moves an attached ``GaussianAdam``'s moments along::

    res = densify_and_prune(params, stats, opt, scene_scale=extent)
    params, stats = res.params, res.stats          # opt's groups already hold res.params

``densify_and_prune_torch`` is the definition (plain torch, any device); ``backend="hip"`` runs csrc/densify.hip
(``ms_densify_classify``, ``ms_densify_move``): three kernels and one host read, no atomics, bitwise reproducible.

Thresholds are formed once on the host in double and rounded to float32; every comparison is float32 and the scale tests
happen in log space (no ``exp`` is taken for a decision), so both backends decide bit-identically.  With
``smax = scales.max(-1)``, ``g = stats.mean_grad()``, ``high = g > grow_grad2d`` and ``small = smax <= log(grow_scale3d *
scene_scale)``:

    clone    = high & small
    split    = (high & ~small) | (max_radii > grow_scale2d)
    lowop    = opacity < prune_opa                      (its logit with opacity_space="logit")
    big      = (smax > log(prune_scale3d * scene_scale)) | (max_radii > prune_scale2d)
    childbig = (smax - log 1.6 > log(prune_scale3d * scene_scale)) | (max_radii > prune_scale2d)

Output rows, each segment in ascending source row: originals with ``~split & ~lowop & ~big``; clones with ``clone & ~lowop
& ~big``; first children with ``split & ~lowop & ~childbig``; second children, the same rows.  This is gsplat's "duplicate,
then split, then prune" in one pass (a row can be cloned and split at once, as there; children inherit their parent's
radius for the prune test).  A clone or an original is a bit copy of every tensor's row; a child copies every row except
``scales = scales[i] - log 1.6`` and ``means3d = means3d[i] + R(q_i / |q_i|) @ (exp(scales[i]) * noise[c, i])``.

The schedule stays with the caller: when to refine, when the screen-size rules stop, when the too-big rule starts
counting -- a rule passed as ``None`` is off.  Not covered: absgrad, gsplat's ``revised_opacity``, a cap on the Gaussian
count (mcmc.py's ``grow`` has one), the sharded trainer, graph capture, float16 parameters.
"""
import ctypes
import math
import struct
from dataclasses import dataclass
from typing import Dict

import torch

from .densify import DensifyStats

REQUIRED = ("means3d", "scales", "quats", "opacities")


def _f32(x: float) -> float:
    """x rounded to float32, as a Python float (so that a float32 comparison against it is exact on every backend)."""
    return struct.unpack("f", struct.pack("f", x))[0]


LOG16 = _f32(math.log(1.6))


@dataclass
class DensifyResult:
    params: Dict[str, torch.Tensor]     # new leaf tensors, requires_grad as the inputs had it
    stats: DensifyStats                 # zeroed, of the new N
    source: torch.Tensor                # int64: each output row's source row
    n_kept: int
    n_cloned: int
    n_split: int                        # split rows; each leaves two children
    n_pruned: int                       # source rows that produce no output row


def _thresholds(grow_grad2d, grow_scale3d, grow_scale2d, prune_opa, prune_scale3d, prune_scale2d, scene_scale, opacity_space):
    """The six float32 thresholds (Python floats holding float32 values); a rule that is off is +inf."""
    inf = float("inf")
    return dict(
        grow_grad2d=_f32(grow_grad2d),
        log_grow=_f32(math.log(grow_scale3d * scene_scale)),
        grow_radius=inf if grow_scale2d is None else _f32(grow_scale2d),
        thr_opa=_f32(prune_opa) if opacity_space == "linear" else _f32(math.log(prune_opa / (1.0 - prune_opa))),
        log_big=inf if prune_scale3d is None else _f32(math.log(prune_scale3d * scene_scale)),
        prune_radius=inf if prune_scale2d is None else _f32(prune_scale2d))


def classify_torch(scales, opacities, stats, thr):
    """-> (original stays, a clone appears, two children appear): three boolean (N,) masks, decided in float32."""
    smax = scales.detach().float().max(-1).values
    opa = opacities.detach().float().reshape(-1)
    rad = stats.max_radii
    high = stats.mean_grad() > thr["grow_grad2d"]
    small = smax <= thr["log_grow"]
    clone = high & small
    split = (high & ~small) | (rad > thr["grow_radius"])
    lowop = opa < thr["thr_opa"]
    rad_big = rad > thr["prune_radius"]
    big = (smax > thr["log_big"]) | rad_big
    childbig = ((smax - LOG16) > thr["log_big"]) | rad_big
    return ~split & ~lowop & ~big, clone & ~lowop & ~big, split & ~lowop & ~childbig


def child_means_torch(means3d, scales, quats, noise):
    """means3d + R(quats / |quats|) @ (exp(scales) * noise), row by row, in the dtype of ``means3d``; quats are wxyz."""
    dt = means3d.dtype
    q = quats.to(dt)
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
    v = torch.exp(scales.to(dt)) * noise.to(dt)
    return means3d + (R * v.unsqueeze(-2)).sum(-1)


def _validate_params(params, opacity_space, backend):
    """The checks of the scene dict itself (densify_and_prune and mcmc.py share them); -> (N, device)."""
    if backend not in ("hip", "torch"):
        raise ValueError(f"Invalid backend: {backend!r} (\"hip\" or \"torch\")")
    if opacity_space not in ("linear", "logit"):
        raise ValueError(f"Invalid opacity_space: {opacity_space!r} (\"linear\" or \"logit\")")
    if not isinstance(params, dict):
        raise ValueError("params must be a dict {name: tensor}")
    missing = [n for n in REQUIRED if n not in params]
    if missing:
        raise ValueError(f"params lacks {missing}: means3d, scales, quats and opacities are required")
    for n, p in params.items():
        if not isinstance(p, torch.Tensor) or p.dim() == 0 or not p.is_floating_point():
            raise ValueError(f"parameter {n!r} must be a floating-point tensor with one row per Gaussian")
    N, dev = params["means3d"].shape[0], params["means3d"].device
    for n, p in params.items():
        if p.shape[0] != N:
            raise ValueError(f"parameter {n!r} has {p.shape[0]} rows, means3d has {N}")
        if p.device != dev:
            raise ValueError(f"parameter {n!r} is on {p.device}, means3d on {dev}")
    for n, shape in (("means3d", (N, 3)), ("scales", (N, 3)), ("quats", (N, 4))):
        if tuple(params[n].shape) != shape:
            raise ValueError(f"parameter {n!r} has shape {tuple(params[n].shape)}, expected {shape}")
    if tuple(params["opacities"].shape) not in ((N,), (N, 1)):
        raise ValueError(f"parameter 'opacities' has shape {tuple(params['opacities'].shape)}, expected ({N},) or ({N}, 1)")
    return N, dev


def _validate_opt(params, opt):
    """opt is None or a GaussianAdam over exactly the tensors of params."""
    from .optim import GaussianAdam
    if opt is not None:
        if not isinstance(opt, GaussianAdam):
            raise ValueError("opt must be a GaussianAdam (or None)")
        names = [g.get("name") for g in opt.param_groups]
        if sorted(names) != sorted(params) or any(len(g["params"]) != 1 or g["params"][0] is not params[g["name"]]
                                                  for g in opt.param_groups):
            raise ValueError(f"opt's groups {names} are not exactly the tensors of params {list(params)}")


def _validate_hip(params, opt, dev):
    """What backend="hip" asks of the parameters and of opt's moments."""
    from .optim import _check_hip_params
    _check_hip_params(list(params.items()))
    for n, p in params.items():
        st = opt.state.get(p) if opt is not None else None
        if st and any(st[k].device != dev for k in ("exp_avg", "exp_avg_sq")):
            raise ValueError(f"backend='hip': the moments of {n!r} are not on {dev}")


def _validate(params, stats, opt, noise, opacity_space, backend):
    """Every check of densify_and_prune; -> (N, device).  Raises ValueError; changes nothing."""
    N, dev = _validate_params(params, opacity_space, backend)
    if not isinstance(stats, DensifyStats):
        raise ValueError("stats must be a DensifyStats")
    stats.check(N, dev)
    if noise is not None:
        if not isinstance(noise, torch.Tensor) or tuple(noise.shape) != (2, N, 3) or noise.dtype != torch.float32 or noise.device != dev:
            raise ValueError(f"noise must be a float32 tensor of shape (2, {N}, 3) on {dev}")
    _validate_opt(params, opt)
    if backend == "hip":
        _validate_hip(params, opt, dev)
        if noise is not None and not noise.is_contiguous():
            raise ValueError("backend='hip': noise must be contiguous")
    return N, dev


def _draw_noise(N, dev, generator):
    return torch.randn((2, N, 3), generator=generator, device=dev, dtype=torch.float32)


def _result(new, params, source, counts, dev):
    for n in new:
        new[n].requires_grad_(params[n].requires_grad)
    n_kept, n_cloned, n_split, n_pruned = counts
    return DensifyResult(new, DensifyStats(n_kept + n_cloned + 2 * n_split, dev), source, n_kept, n_cloned, n_split, n_pruned)


@torch.no_grad()
def densify_and_prune_torch(params, stats, opt=None, *, thr, noise):
    """THE DEFINITION, on inputs ``_validate`` has passed: ``thr`` from ``_thresholds``, ``noise`` (2, N, 3) float32."""
    N, dev = params["means3d"].shape[0], params["means3d"].device
    keep, cloned, split = classify_torch(params["scales"], params["opacities"], stats, thr)
    rows = torch.arange(N, device=dev)
    i_keep, i_clone, i_split = rows[keep], rows[cloned], rows[split]
    source = torch.cat([i_keep, i_clone, i_split, i_split])
    first = i_keep.numel() + i_clone.numel()            # the first child's row
    new = {n: p.detach()[source].contiguous() for n, p in params.items()}
    new["scales"][first:] = params["scales"].detach()[source[first:]] - LOG16
    S = i_split.numel()
    for c in range(2):
        new["means3d"][first + c * S: first + (c + 1) * S] = child_means_torch(
            params["means3d"].detach()[i_split], params["scales"].detach()[i_split], params["quats"].detach()[i_split],
            noise[c][i_split])
    res = _result(new, params, source, (i_keep.numel(), i_clone.numel(), S, N - int((keep | cloned | split).sum())), dev)
    if opt is not None:
        opt.relocate(res.params, keep, i_clone.numel() + 2 * S)
    return res


@torch.no_grad()
def _densify_and_prune_hip(params, stats, opt, thr, noise):
    from . import _hip
    from .binning import _pinned_info
    N, dev = params["means3d"].shape[0], params["means3d"].device
    L = _hip.lib()
    names = list(params)
    moments = {}                                        # name -> [exp_avg, exp_avg_sq] of the parameters that have state
    if opt is not None:
        for n in names:
            st = opt.state.get(params[n])
            if st:
                moments[n] = [_hip.f32c(st["exp_avg"]), _hip.f32c(st["exp_avg_sq"])]
    counts = (0, 0, 0, 0)
    with _hip.on_device(dev):
        stream = _hip.stream(dev)
        if N:
            ws = torch.empty(L.ms_densify_workspace_bytes(N), dtype=torch.uint8, device=dev)
            totals = torch.empty(4, dtype=torch.int64, device=dev)
            rules = _hip.DensifyRules(**thr)
            _hip.check(L.ms_densify_classify(N, _hip.ptr(stats.grad2d), _hip.ptr(stats.count), _hip.ptr(stats.max_radii),
                                             _hip.ptr(params["scales"]), _hip.ptr(params["opacities"]), ctypes.byref(rules),
                                             _hip.ptr(ws), ws.numel(), _hip.ptr(totals), stream), "ms_densify_classify")
            host = _pinned_info(dev)
            host[:4].copy_(totals, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()        # the one host wait: the outputs have to be allocated
            counts = tuple(int(v) for v in host[:4].tolist())
        n_kept, n_cloned, n_split, _ = counts
        n_out = n_kept + n_cloned + 2 * n_split
        out = lambda t: torch.empty((n_out, *t.shape[1:]), dtype=torch.float32, device=dev)
        new = {n: out(params[n]) for n in names}
        new_moments = {n: [out(m) for m in ms_] for n, ms_ in moments.items()}
        source = torch.empty(n_out, dtype=torch.int64, device=dev)
        if n_out:
            kinds = {"means3d": _hip.DENSIFY_MEAN, "scales": _hip.DENSIFY_SCALE}
            work = []                                   # (src, dst, width, kind)
            for n in names:
                width = params[n].numel() // N
                if width == 0:
                    continue
                work.append((params[n], new[n], width, kinds.get(n, _hip.DENSIFY_COPY)))
                for m, nm in zip(moments.get(n, ()), new_moments.get(n, ())):
                    work.append((m, nm, width, _hip.DENSIFY_MOMENT))
            for c0 in range(0, len(work), _hip.DENSIFY_MAX_TENSORS):
                chunk = work[c0:c0 + _hip.DENSIFY_MAX_TENSORS]
                table = (_hip.DensifyTensor * len(chunk))()
                for rec, (src, dst, width, kind) in zip(table, chunk):
                    rec.src, rec.dst, rec.width, rec.kind = src.data_ptr(), dst.data_ptr(), width, kind
                # the first launch also writes `source` and the children's means
                row_args = [_hip.ptr(t) for t in (params["means3d"], params["scales"], params["quats"], noise, new["means3d"], source)] \
                    if c0 == 0 else [None] * 6
                _hip.check(L.ms_densify_move(N, n_kept, n_cloned, n_split, _hip.ptr(ws), ws.numel(), len(chunk), table,
                                             *row_args, stream), "ms_densify_move")
    res = _result(new, params, source, counts, dev)
    if opt is not None:
        opt._adopt(res.params, new_moments)
    return res


def densify_and_prune(params, stats, opt=None, *, grow_grad2d=2e-4, grow_scale3d=0.01, grow_scale2d=0.05, prune_opa=0.005,
                      prune_scale3d=0.1, prune_scale2d=0.15, scene_scale=1.0, opacity_space="linear", noise=None,
                      generator=None, backend="hip") -> DensifyResult:
    """Clone, split and prune the scene ``params`` from ``stats`` (module docstring), moving ``opt``'s moments along.

    params: {name: tensor} with N rows each; "means3d" (N, 3), "scales" (N, 3, log space), "quats" (N, 4, wxyz) and
    "opacities" (N,) or (N, 1) are required, any other name (any width or shape) is carried along.  stats: the
    DensifyStats of these N Gaussians.  opt: a GaussianAdam over exactly these tensors, or None: its groups adopt the new
    tensors, its moments become ``old[row]`` for surviving originals and zero for every clone and child (``step`` is kept)
    -- ``opt.relocate(res.params, keep_mask, n_cloned + 2 * n_split)``.  grow_scale2d, prune_scale3d, prune_scale2d: None
    switches the rule off.  opacity_space: what "opacities" holds, "linear" or "logit".  noise: (2, N, 3) float32 standard
    normal, drawn with ``torch.randn(generator=generator)`` when None.

    backend="hip": CUDA/ROCm, float32, contiguous tensors on one device; one host wait (the three totals); no fallback.
    Every check happens before anything is changed (ValueError)."""
    N, dev = _validate(params, stats, opt, noise, opacity_space, backend)
    for name, v in (("grow_grad2d", grow_grad2d), ("grow_scale3d", grow_scale3d), ("prune_opa", prune_opa), ("scene_scale", scene_scale),
                    ("grow_scale2d", grow_scale2d), ("prune_scale3d", prune_scale3d), ("prune_scale2d", prune_scale2d)):
        if v is not None and not (math.isfinite(v) and v > 0.0):
            raise ValueError(f"{name} must be positive and finite, got {v}")
    if opacity_space == "logit" and not prune_opa < 1.0:
        raise ValueError(f"prune_opa must lie in (0, 1) in logit space, got {prune_opa}")
    thr = _thresholds(grow_grad2d, grow_scale3d, grow_scale2d, prune_opa, prune_scale3d, prune_scale2d, scene_scale, opacity_space)
    if backend == "hip":
        from . import _hip
        _hip.lib()                                      # (a missing library or GPU is an error before anything moves)
    if noise is None:
        noise = _draw_noise(N, dev, generator)
    if backend == "torch":
        return densify_and_prune_torch(params, stats, opt, thr=thr, noise=noise)
    return _densify_and_prune_hip(params, stats, opt, thr, noise)


@torch.no_grad()
def reset_opacities(opacities, opt=None, max_opacity=0.01, opacity_space="linear"):
    """3DGS's opacity reset: clamp ``opacities`` in place to at most ``max_opacity`` (its logit with
    opacity_space="logit") and zero the moments of the group of ``opt`` that holds this tensor."""
    if opacity_space not in ("linear", "logit"):
        raise ValueError(f"Invalid opacity_space: {opacity_space!r} (\"linear\" or \"logit\")")
    if not 0.0 < max_opacity < 1.0:
        raise ValueError(f"max_opacity must lie in (0, 1), got {max_opacity}")
    name = None
    if opt is not None:
        name = next((g.get("name") for g in opt.param_groups if any(p is opacities for p in g["params"])), None)
        if name is None:
            raise ValueError("reset_opacities: opt holds no group with this tensor")
    opacities.clamp_(max=max_opacity if opacity_space == "linear" else math.log(max_opacity / (1.0 - max_opacity)))
    if opt is not None:
        opt.zero_state(name)
    return opacities


__all__ = ["densify_and_prune", "densify_and_prune_torch", "reset_opacities", "DensifyResult", "classify_torch",
           "child_means_torch", "LOG16"]
