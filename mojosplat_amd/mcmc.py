"""The MCMC strategy of 3D Gaussian Splatting training: relocate dead Gaussians, grow the scene, perturb the means.

3DGS-MCMC (Kheradmand et al. 2024; gsplat's ``MCMCStrategy``) keeps a budget of Gaussians instead of cloning, splitting
and pruning: a dead Gaussian is teleported onto a live one sampled by opacity, the scene grows by 5 % at a time up to a cap
the same way, and after every optimiser step the means take a step of covariance-shaped noise::

    opt.step(); opt.zero_grad()
    inject_noise(params, lr=opt.group("means3d")["lr"])
    if step % 100 == 0:
        relocate_dead(params, opt)
        params = grow(params, opt, cap_max=1_000_000).params     # opt's groups already hold the new tensors

``relocate_dead_torch``, ``grow_torch`` and ``inject_noise_torch`` are the definition (plain torch, any device and float
dtype); ``backend="hip"`` runs csrc/mcmc.hip (``ms_mcmc_sample``, ``ms_mcmc_apply``, ``ms_mcmc_noise``) and makes no host
wait: the number of dead rows stays on the device.

OPACITY AND THE DEAD RULE.  ``o = opacities`` (opacity_space="linear") or ``sigmoid(opacities)`` ("logit"), float32.  A row
is dead when ``not (opacities > thr)`` on the STORED value, ``thr = float32(min_opacity)`` or ``float32(logit(min_opacity))``:
both backends decide bit-identically and a NaN is dead.

SAMPLING, exact in integers.  ``w_i = 0`` for a dead row, else ``int64(round(o_i * 2**24))`` (the product is exact);
``cum = cumsum(w)``, ``total = cum[-1]``.  Draw ``j`` takes ``u_j`` from ``draws`` (float64 uniforms in [0, 1);
``torch.rand(dtype=float64, generator=generator)`` when None): ``t_j = min(int64(floor(u_j * total)), total - 1)`` and
``sampled_j = searchsorted(cum, t_j, right=True)``, never a zero-weight row.  ``sampled=`` (int64) bypasses the draw (a
caller's own sampler; comparing backends in logit space, where two ``exp`` may differ by an ulp).  A draw whose source is
not a live row (out of range, dead, or any draw when ``total == 0``) is NOT APPLIED and reported as ``sampled_j = -1``.

NEW VALUES.  With ``c_i`` applied draws of source ``i`` and ``n = min(1 + c_i, 51)``::

    o' = -expm1(log1p(-o_i) / n)
    D  = sum_{a=1..n} sum_{b=0..a-1} C(a-1, b) (-1)^b / sqrt(b+1) o'^(b+1) = sum_{b=0..n-1} K[n-1][b] o'^(b+1)
    scales_i += log(o_i / D);   opacity_i = clamp(o', min_opacity, 1 - 1e-7)   (stored as its logit in logit space)

``K[n-1][b] = (-1)^b C(n, b+1) / sqrt(b+1)`` is the inner sum over ``a`` carried out (sum_{a=b+1..n} C(a-1, b) =
C(n, b+1)): ``BINOM``, 51 x 51, formed in double and rounded to float32 ONCE; both backends and every dtype read that table.
The sum is evaluated by Horner's rule.  The rendered image is preserved: ``n`` Gaussians of opacity ``o'`` at one place
composite to ``o``, and the scale keeps the footprint's integral.

``relocate_dead``: the dead rows in ascending order are the targets, draw ``j`` belongs to target ``j`` (``draws`` has N
entries, the first ``n_dead`` are used -- this is what spares the host the count).  Every source takes its new values;
every target becomes a bit copy of every tensor's row of its source, with those same values; the moments of all sources and
all targets become ZERO (gsplat leaves the targets' moments: a dead row's moments describe a Gaussian that no longer
exists); ``step`` is kept.  In place, N unchanged.  ``sampled`` and ``targets`` have N entries, -1 from ``n`` on; ``n`` is a
device int64 scalar.  ``total == 0`` or no dead row: nothing is done.

``grow``: ``n_new = max(0, min(cap_max, int(growth * N)) - N)`` draws over the same weights, sources rewritten as above,
row ``N + j`` a copy of row ``sampled_j`` with the new values; new leaf tensors (``requires_grad`` as the inputs), moments
``opt.relocate(new, arange(N), n_new)`` with the sources' rows zeroed.  Because nothing waits for ``total``, the row of a
draw that is not applied is a copy of row 0 and rewrites nothing (with ``total == 0`` that is every new row: all dead).

``inject_noise``: ``means3d += Sigma @ (noise * gate * (lr * noise_lr))`` in place, ``Sigma = R diag(exp(2 scales)) R^T``
with ``R = R(quats / |quats|)``, evaluated as ``R (exp(2 scales) * (R^T v))`` (the 3 x 3 product is never formed, so
nothing cancels), ``gate = 1 / (1 + exp(-k ((1 - o) - x0)))``, ``noise`` (N, 3) float32 standard normal.

Not covered: the sharded trainer, graph capture, float16 parameters, and the opacity and scale regularisers of the paper
(``lambda_o * o.mean()`` and ``lambda_s * exp(scales).mean()``: two torch means in the caller's loss).
"""
import math
from dataclasses import dataclass
from typing import Dict, Union

import torch

from .refine import _f32, _validate_hip, _validate_opt, _validate_params

MAX_RATIO = 51
SCALE24 = 16777216.0
MAX_OPACITY = 1.0 - 1e-7
KEYS = ("exp_avg", "exp_avg_sq")


def _binom_table():
    K = torch.zeros((MAX_RATIO, MAX_RATIO), dtype=torch.float64)
    for n in range(1, MAX_RATIO + 1):
        for b in range(n):
            K[n - 1, b] = (-1.0) ** b * math.comb(n, b + 1) / math.sqrt(b + 1.0)
    return K.float()


BINOM = _binom_table()          # K[n-1][b] of the module docstring, float32
_binom_on = {}


def _binom(device):
    if device.type == "cpu":
        return BINOM
    if device not in _binom_on:
        _binom_on[device] = BINOM.to(device)
    return _binom_on[device]


@dataclass
class McmcResult:
    params: Dict[str, torch.Tensor]     # relocate_dead: the inputs, updated in place; grow: new leaf tensors
    sampled: torch.Tensor               # int64: the source row of each draw (-1: the draw was not applied)
    targets: torch.Tensor               # int64: the row each draw was written to (-1: past the last draw)
    n: Union[int, torch.Tensor]         # the draws made: relocate_dead: a device int64 scalar (no host wait); grow: an int


def _threshold(min_opacity, opacity_space):
    return _f32(min_opacity) if opacity_space == "linear" else _f32(math.log(min_opacity / (1.0 - min_opacity)))


def dead_and_cum_torch(opacities, min_opacity, opacity_space):
    """-> (dead (N,) bool, cum (N,) int64): the dead rule on the stored values and the scan of the integer weights."""
    x = opacities.detach().reshape(-1)
    dead = ~(x > _threshold(min_opacity, opacity_space))
    o = x.float()
    if opacity_space == "logit":
        o = torch.sigmoid(o)
    w = torch.where(dead, torch.zeros_like(o), torch.round(o * SCALE24)).to(torch.int64)
    return dead, torch.cumsum(w, 0)


def sample_torch(cum, dead, draws):
    """draws (float64 uniforms) -> int64 source rows; -1 where the draw cannot be applied."""
    total = int(cum[-1])
    if total <= 0:
        return torch.full(draws.shape, -1, dtype=torch.int64, device=draws.device)
    t = torch.clamp((draws * total).floor().to(torch.int64), max=total - 1)
    s = torch.searchsorted(cum, t, right=True).clamp(max=cum.numel() - 1)
    return torch.where(dead[s], torch.full_like(s, -1), s)


def _checked(sampled, dead):
    """A caller's own draws: -1 where the source is out of range or dead."""
    N = dead.numel()
    ok = (sampled >= 0) & (sampled < N)
    ok &= ~dead[sampled.clamp(0, N - 1)]
    return torch.where(ok, sampled, torch.full_like(sampled, -1))


def relocated_torch(o, n, min_opacity=0.005):
    """The new values of sources of opacity ``o`` (linear) that stand for ``n`` (int64, >= 1; above 51 counts as 51)
    Gaussians each -> (o' clamped to [min_opacity, 1 - 1e-7], log(o / D)), in the dtype of ``o``."""
    dt = o.dtype
    n = n.clamp(max=MAX_RATIO)
    op = -torch.expm1(torch.log1p(-o) / n.to(dt))
    K = _binom(o.device).to(dt)[n - 1]
    acc = torch.zeros_like(o)
    for b in range(MAX_RATIO - 1, -1, -1):
        acc = acc * op + K[..., b]
    return op.clamp(min_opacity, MAX_OPACITY), torch.log(o / (acc * op))


def _moments(params, opt):
    """{name: state} of the parameters of ``opt`` that have moments."""
    out = {}
    if opt is not None:
        for n, p in params.items():
            st = opt.state.get(p)
            if st:
                out[n] = st
    return out


def _rewrite_sources_torch(params, moments, sampled, min_opacity, opacity_space):
    """The sources among ``sampled`` (-1: no draw) take their new opacity and scale and lose their moments, in place."""
    N = params["means3d"].shape[0]
    counts = torch.bincount(sampled[sampled >= 0], minlength=N)
    src = torch.nonzero(counts).reshape(-1)
    if src.numel() == 0:
        return
    opa, scales = params["opacities"].detach().view(N), params["scales"].detach()
    dt = opa.dtype
    o = opa[src]
    if opacity_space == "logit":
        o = torch.sigmoid(o)
    o_new, dlog = relocated_torch(o, counts[src] + 1, min_opacity)
    opa[src] = torch.log(o_new / (1.0 - o_new)) if opacity_space == "logit" else o_new
    scales[src] = (scales[src].to(dt) + dlog.unsqueeze(-1)).to(scales.dtype)
    for st in moments.values():
        for k in KEYS:
            st[k][src] = 0


@torch.no_grad()
def relocate_dead_torch(params, opt=None, *, min_opacity, opacity_space, draws, sampled=None):
    """THE DEFINITION, on inputs ``_validate`` has passed; ``draws`` (N,) float64 or ``sampled`` (N,) int64."""
    N, dev = params["means3d"].shape[0], params["means3d"].device
    pad = lambda v: torch.cat([v, torch.full((N - v.numel(),), -1, dtype=torch.int64, device=dev)])
    dead, cum = dead_and_cum_torch(params["opacities"], min_opacity, opacity_space)
    targets = torch.nonzero(dead).reshape(-1)
    n = targets.numel() if N and int(cum[-1]) > 0 else 0
    targets = targets[:n]
    s = _checked(sampled[:n], dead) if sampled is not None else sample_torch(cum, dead, draws[:n]) if n else targets
    moments = _moments(params, opt)
    _rewrite_sources_torch(params, moments, s, min_opacity, opacity_space)
    ok = s >= 0
    src, dst = s[ok], targets[ok]
    for name, p in params.items():
        p.detach()[dst] = p.detach()[src]
        if name in moments:
            for k in KEYS:
                moments[name][k][dst] = 0
    return McmcResult(params, pad(s), pad(targets), torch.tensor(n, dtype=torch.int64, device=dev))


def _n_new(N, cap_max, growth):
    return max(0, min(int(cap_max), int(growth * N)) - N)


@torch.no_grad()
def grow_torch(params, opt=None, *, n_new, min_opacity, opacity_space, draws, sampled=None):
    """THE DEFINITION, on inputs ``_validate`` has passed; ``draws`` (n_new,) float64 or ``sampled`` (n_new,) int64."""
    N, dev = params["means3d"].shape[0], params["means3d"].device
    dead, cum = dead_and_cum_torch(params["opacities"], min_opacity, opacity_space)
    s = _checked(sampled, dead) if sampled is not None else sample_torch(cum, dead, draws)
    new = {n: torch.cat([p.detach(), p.detach().new_empty((n_new, *p.shape[1:]))]) for n, p in params.items()}
    for n in new:
        new[n].requires_grad_(params[n].requires_grad)
    if opt is not None:
        opt.relocate(new, torch.arange(N, device=dev), n_new)
    _rewrite_sources_torch(new, _moments(new, opt), s, min_opacity, opacity_space)
    src = s.clamp(min=0)                                # (a draw that was not applied: a copy of row 0)
    for p in new.values():
        p.detach()[N:] = p.detach()[src]
    return McmcResult(new, s, torch.arange(N, N + n_new, device=dev), n_new)


def rotation_torch(quats):
    """R(q / |q|), (N, 3, 3), in the dtype of ``quats``; wxyz."""
    q = quats / quats.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)


def noise_step_torch(scales, quats, opacities, noise, step, opacity_space="logit", k=100.0, x0=0.995):
    """Sigma @ (noise * gate * step), (N, 3), in the dtype of ``scales``, evaluated as R (exp(2 scales) * (R^T v))."""
    dt = scales.dtype
    R = rotation_torch(quats.to(dt))
    o = opacities.reshape(-1).to(dt)
    if opacity_space == "logit":
        o = torch.sigmoid(o)
    gate = 1.0 / (1.0 + torch.exp(-k * ((1.0 - o) - x0)))
    v = (noise.to(dt) * gate.unsqueeze(-1)) * step
    local = torch.exp(2.0 * scales) * (R * v.unsqueeze(-1)).sum(-2)          # exp(2 s) * (R^T v)
    return (R * local.unsqueeze(-2)).sum(-1)


@torch.no_grad()
def inject_noise_torch(params, lr, *, noise, noise_lr=5e5, opacity_space="logit", k=100.0, x0=0.995):
    """THE DEFINITION, on inputs ``_validate`` has passed, in the dtype of ``means3d``; in place."""
    m = params["means3d"].detach()
    dt = m.dtype
    m.add_(noise_step_torch(params["scales"].detach().to(dt), params["quats"].detach(), params["opacities"].detach(), noise,
                            lr * noise_lr, opacity_space, k, x0))


# ---------------------------------------------------------------------------------------------------------- checks
def _validate(params, opt, opacity_space, backend, min_opacity=0.005):
    N, dev = _validate_params(params, opacity_space, backend)
    if not (isinstance(min_opacity, (int, float)) and 0.0 < min_opacity < 1.0):
        raise ValueError(f"min_opacity must lie in (0, 1), got {min_opacity}")
    _validate_opt(params, opt)
    if backend == "hip":
        _validate_hip(params, opt, dev)
        for n, p in params.items():
            if p.numel() >= 2 ** 31:
                raise ValueError(f"backend='hip': parameter {n!r} has 2^31 elements or more")
    return N, dev


def _check_draws(draws, sampled, n, dev, backend):
    for name, t, dtype in (("draws", draws, torch.float64), ("sampled", sampled, torch.int64)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (n,) or t.dtype != dtype or t.device != dev:
            raise ValueError(f"{name} must be a {str(dtype).replace('torch.', '')} tensor of shape ({n},) on {dev}")
        if backend == "hip" and not t.is_contiguous():
            raise ValueError(f"backend='hip': {name} must be contiguous")


# ---------------------------------------------------------------------------------------------------------- backend="hip"
def _apply_hip(L, _hip, tensors, moments, N, n_draws, n_rows, grow, ws, sampled, targets, logit, min_opacity, dev, stream):
    """ms_mcmc_apply over every tensor of ``tensors`` {name: (n_rows, ...)} and ``moments`` {name: [exp_avg, exp_avg_sq]}."""
    kinds = {"opacities": _hip.MCMC_OPACITY, "scales": _hip.MCMC_SCALE}
    work = []                                           # (tensor, width, kind)
    for n, p in tensors.items():
        width = p.numel() // n_rows
        if width == 0:
            continue
        work.append((p, width, kinds.get(n, _hip.MCMC_COPY)))
        work.extend((m, width, _hip.MCMC_MOMENT) for m in moments.get(n, ()))
    binom = _binom(dev)
    for c0 in range(0, len(work), _hip.MCMC_MAX_TENSORS):
        chunk = work[c0:c0 + _hip.MCMC_MAX_TENSORS]
        table = (_hip.McmcTensor * len(chunk))()
        for rec, (t, width, kind) in zip(table, chunk):
            rec.base, rec.width, rec.kind = t.data_ptr(), width, kind
        # the first launch also computes every row's new values, from the values as they still are
        value_args = [_hip.ptr(t) for t in (tensors["opacities"], tensors["scales"], binom)] if c0 == 0 else [None] * 3
        _hip.check(L.ms_mcmc_apply(N, n_draws, n_rows, grow, _hip.ptr(ws), ws.numel(), _hip.ptr(sampled), _hip.ptr(targets),
                                   len(chunk), table, *value_args, logit, min_opacity, stream), "ms_mcmc_apply")


def _hip_moments(params, opt, _hip):
    """{name: [exp_avg, exp_avg_sq]}, float32 and contiguous (a loaded state dict's are converted in the state itself)."""
    out = {}
    for n, st in _moments(params, opt).items():
        for k in KEYS:
            if st[k].dtype != torch.float32 or not st[k].is_contiguous():
                st[k] = _hip.f32c(st[k])
        out[n] = [st[k] for k in KEYS]
    return out


@torch.no_grad()
def _relocate_dead_hip(params, opt, N, dev, min_opacity, opacity_space, draws, sampled):
    from . import _hip
    L = _hip.lib()
    logit = int(opacity_space == "logit")
    out_s = torch.empty(N, dtype=torch.int64, device=dev)
    out_t = torch.empty(N, dtype=torch.int64, device=dev)
    n = torch.zeros((), dtype=torch.int64, device=dev)
    if N:
        moments = _hip_moments(params, opt, _hip)
        with _hip.on_device(dev):
            stream = _hip.stream(dev)
            ws = torch.empty(L.ms_mcmc_workspace_bytes(N), dtype=torch.uint8, device=dev)
            _hip.check(L.ms_mcmc_sample(N, _hip.ptr(params["opacities"]), logit, _threshold(min_opacity, opacity_space), N, 0,
                                        _hip.ptr(draws), _hip.ptr(sampled), _hip.ptr(ws), ws.numel(), _hip.ptr(out_s),
                                        _hip.ptr(out_t), _hip.ptr(n), stream), "ms_mcmc_sample")
            _apply_hip(L, _hip, params, moments, N, N, N, 0, ws, out_s, out_t, logit, min_opacity, dev, stream)
        # (written through raw pointers: the version counters move where relocate_dead_torch's index assignments move them)
        _hip.bump(*params.values(), *[m for ms_ in moments.values() for m in ms_])
    return McmcResult(params, out_s, out_t, n)


@torch.no_grad()
def _grow_hip(params, opt, N, dev, n_new, min_opacity, opacity_space, draws, sampled):
    from . import _hip
    L = _hip.lib()
    logit = int(opacity_space == "logit")
    out_s = torch.empty(n_new, dtype=torch.int64, device=dev)
    out_t = torch.empty(n_new, dtype=torch.int64, device=dev)

    def longer(t):                                      # rows [0, N) copied, the kernel writes the rest
        out = torch.empty((N + n_new, *t.shape[1:]), dtype=torch.float32, device=dev)
        out[:N].copy_(t.detach())
        return out

    new = {n: longer(p) for n, p in params.items()}
    moments = {n: [longer(m) for m in ms_] for n, ms_ in _hip_moments(params, opt, _hip).items()}
    with _hip.on_device(dev):
        stream = _hip.stream(dev)
        ws = torch.empty(L.ms_mcmc_workspace_bytes(N), dtype=torch.uint8, device=dev)
        _hip.check(L.ms_mcmc_sample(N, _hip.ptr(params["opacities"]), logit, _threshold(min_opacity, opacity_space), n_new, 1,
                                    _hip.ptr(draws), _hip.ptr(sampled), _hip.ptr(ws), ws.numel(), _hip.ptr(out_s),
                                    _hip.ptr(out_t), None, stream), "ms_mcmc_sample")
        _apply_hip(L, _hip, new, moments, N, n_new, N + n_new, 1, ws, out_s, out_t, logit, min_opacity, dev, stream)
    for n in new:
        new[n].requires_grad_(params[n].requires_grad)
    if opt is not None:
        opt._adopt(new, moments)
    return McmcResult(new, out_s, out_t, n_new)


# ---------------------------------------------------------------------------------------------------------- public
def relocate_dead(params, opt=None, *, min_opacity=0.005, opacity_space="logit", draws=None, sampled=None, generator=None,
                  backend="hip") -> McmcResult:
    """Teleport every dead Gaussian of ``params`` onto a live one sampled by opacity (module docstring), in place.

    params: {name: tensor} with N rows each, as ``densify_and_prune`` takes it: "means3d" (N, 3), "scales" (N, 3, log
    space), "quats" (N, 4, wxyz) and "opacities" (N,) or (N, 1) are required, any other name is carried along.  opt: a
    GaussianAdam over exactly these tensors, or None: the moments of every source and target become zero, ``step`` is kept.
    draws: (N,) float64 uniforms in [0, 1), the first n_dead are used; sampled: (N,) int64 source rows instead.

    backend="hip": CUDA/ROCm, float32, contiguous tensors on one device; NO host wait (``res.n`` is a device scalar,
    ``res.sampled`` and ``res.targets`` hold -1 from ``n`` on); no fallback.  Every check happens before anything is changed
    (ValueError); the VALUES of ``sampled`` cannot be checked without a wait: a draw whose source is not a live row is skipped."""
    N, dev = _validate(params, opt, opacity_space, backend, min_opacity)
    _check_draws(draws, sampled, N, dev, backend)
    if backend == "hip":
        from . import _hip
        _hip.lib()                                      # (a missing library or GPU is an error before anything moves)
    if draws is None and sampled is None:
        draws = torch.rand(N, dtype=torch.float64, device=dev, generator=generator)
    if backend == "torch":
        return relocate_dead_torch(params, opt, min_opacity=min_opacity, opacity_space=opacity_space, draws=draws, sampled=sampled)
    return _relocate_dead_hip(params, opt, N, dev, min_opacity, opacity_space, draws, sampled)


def grow(params, opt=None, *, cap_max, growth=1.05, min_opacity=0.005, opacity_space="logit", draws=None, sampled=None,
         generator=None, backend="hip") -> McmcResult:
    """Grow the scene to ``min(cap_max, int(growth * N))`` Gaussians: each new row is a copy of a live one sampled by
    opacity, and source and copy share the new opacity and scale (module docstring).

    params, opt, min_opacity, opacity_space, backend: as ``relocate_dead``.  draws / sampled: (n_new,), n_new = ``res.n``.
    Returns new leaf tensors (``requires_grad`` as the inputs had it) that opt's groups already hold; its moments are
    ``opt.relocate(new, arange(N), n_new)`` with the sources' rows zeroed.  ``cap_max <= N`` (or growth <= 1): nothing is
    done and ``res.params is params``.  backend="hip" makes no host wait."""
    N, dev = _validate(params, opt, opacity_space, backend, min_opacity)
    if not (isinstance(cap_max, int) and cap_max >= 0):
        raise ValueError(f"cap_max must be a non-negative int, got {cap_max!r}")
    if not (math.isfinite(growth) and growth > 0.0):
        raise ValueError(f"growth must be positive and finite, got {growth}")
    n_new = _n_new(N, cap_max, growth)
    _check_draws(draws, sampled, n_new, dev, backend)
    if backend == "hip":
        from . import _hip
        _hip.lib()
        if any((N + n_new) * (p.numel() // max(N, 1)) >= 2 ** 31 for p in params.values()):
            raise ValueError("backend='hip': a parameter would have 2^31 elements or more")
    if n_new == 0:
        empty = torch.empty(0, dtype=torch.int64, device=dev)
        return McmcResult(params, empty, empty.clone(), 0)
    if draws is None and sampled is None:
        draws = torch.rand(n_new, dtype=torch.float64, device=dev, generator=generator)
    if backend == "torch":
        return grow_torch(params, opt, n_new=n_new, min_opacity=min_opacity, opacity_space=opacity_space, draws=draws, sampled=sampled)
    return _grow_hip(params, opt, N, dev, n_new, min_opacity, opacity_space, draws, sampled)


def inject_noise(params, lr, *, noise_lr=5e5, opacity_space="logit", k=100.0, x0=0.995, noise=None, generator=None,
                 backend="hip") -> None:
    """``means3d += Sigma @ (noise * gate * (lr * noise_lr))`` in place (module docstring): the exploration step of
    3DGS-MCMC, after every optimiser step.  lr: the learning rate of the means at this step.  noise: (N, 3) float32 standard
    normal, drawn with ``torch.randn(generator=generator)`` when None.  Opaque Gaussians stand still: the gate is
    ``sigmoid(k ((1 - o) - x0))``.  backend="hip": one launch, no scratch, no host wait; no fallback."""
    N, dev = _validate(params, None, opacity_space, backend)
    for name, v in (("lr", lr), ("noise_lr", noise_lr), ("k", k), ("x0", x0)):
        if not (isinstance(v, (int, float)) and math.isfinite(v)):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if noise is not None:
        if not isinstance(noise, torch.Tensor) or tuple(noise.shape) != (N, 3) or noise.dtype != torch.float32 or noise.device != dev:
            raise ValueError(f"noise must be a float32 tensor of shape ({N}, 3) on {dev}")
        if backend == "hip" and not noise.is_contiguous():
            raise ValueError("backend='hip': noise must be contiguous")
    if backend == "hip":
        from . import _hip
        L = _hip.lib()
    if noise is None:
        noise = torch.randn((N, 3), generator=generator, device=dev, dtype=torch.float32)
    if backend == "torch":
        return inject_noise_torch(params, lr, noise=noise, noise_lr=noise_lr, opacity_space=opacity_space, k=k, x0=x0)
    with _hip.on_device(dev):
        _hip.check(L.ms_mcmc_noise(N, _hip.ptr(params["means3d"]), _hip.ptr(params["scales"]), _hip.ptr(params["quats"]),
                                   _hip.ptr(params["opacities"]), _hip.ptr(noise), int(opacity_space == "logit"),
                                   lr * noise_lr, k, x0, _hip.stream(dev)), "ms_mcmc_noise")
    _hip.bump(params["means3d"])                        # (the only tensor the kernel writes, as inject_noise_torch's add_)


__all__ = ["relocate_dead", "grow", "inject_noise", "McmcResult", "relocate_dead_torch", "grow_torch", "inject_noise_torch",
           "relocated_torch", "noise_step_torch", "dead_and_cum_torch", "sample_torch", "BINOM", "MAX_RATIO"]
