"""The parameter update of 3D Gaussian Splatting training: Adam over the named tensors of a scene.

``GaussianAdam`` is ``torch.optim.Adam`` with default flags (no amsgrad, weight decay or maximize), one param group
per named tensor, with the two things a 3DGS trainer needs on top:

* ``step(visibility=mask)``: the "selective" / "sparse" update of Taming-3DGS and gsplat's ``SelectiveAdam``.  A
  Gaussian (row) the view did not see keeps its parameters AND its moments, bit for bit; the bias corrections use the
  global step count;
* ``relocate(new_params, keep, n_new)``: the moments follow a densification (clone, split, prune) the way
  ``DensifyStats.select(keep).append(n_new)`` moves the statistics; ``zero_state(name)`` is the opacity reset.

``backend="torch"`` is the definition (plain torch ops, any device and float dtype); ``backend="hip"`` runs all tensors
of a step in one launch of csrc/adam.hip (``ms_adam_step``)::

    opt = GaussianAdam({"means3d": means3d, "scales": scales, "quats": quats, "opacities": opac, "features": feats},
                       lr={"means3d": 1.6e-4, "scales": 5e-3, "quats": 1e-3, "opacities": 5e-2, "features": 2.5e-3})
    loss.backward()
    opt.step(visibility=radii_of_this_view > 0)     # or opt.step(): dense
    opt.zero_grad()
"""
import math

import torch

_ADAM_FLAGS = None


def _adam_flags():
    """torch.optim.Adam's own defaults of the installed torch, so that a state dict of ours carries every key its
    ``step`` reads (amsgrad, weight_decay, maximize, foreach, capturable, ...)."""
    global _ADAM_FLAGS
    if _ADAM_FLAGS is None:
        _ADAM_FLAGS = dict(torch.optim.Adam([torch.zeros(1)]).defaults)
    return dict(_ADAM_FLAGS)


def adam_update_torch(p, g, m, v, lr, beta1, beta2, eps, t, visible=None):
    """THE DEFINITION: one Adam step (step count ``t`` >= 1) of one tensor, in place, in the tensors' own dtype.

    m' = beta1 m + (1 - beta1) g;  v' = beta2 v + (1 - beta2) g g;
    p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps),  bc1 = 1 - beta1^t, bc2 = 1 - beta2^t (formed in double).
    ``visible``: a boolean (rows,) tensor or None; rows where it is False keep p, m and v untouched."""
    step_size = lr / (1.0 - beta1 ** t)
    bc2_sqrt = math.sqrt(1.0 - beta2 ** t)
    g = g.to(p.dtype)
    m_new = beta1 * m + (1.0 - beta1) * g
    v_new = beta2 * v + ((1.0 - beta2) * g) * g
    p_new = p - (step_size * m_new) / (v_new.sqrt() / bc2_sqrt + eps)
    if visible is not None:
        sel = visible.view(-1, *([1] * (p.dim() - 1)))
        p_new, m_new, v_new = torch.where(sel, p_new, p), torch.where(sel, m_new, m), torch.where(sel, v_new, v)
    p.copy_(p_new)
    m.copy_(m_new)
    v.copy_(v_new)


class GaussianAdam(torch.optim.Optimizer):
    """Adam over ``params = {name: tensor}``, one param group per name (kept in the group as ``"name"``).

    lr: a float, or a dict that covers every name.  ``lr``, ``betas`` and ``eps`` are read from ``param_groups`` on
    every step (learning-rate schedulers work).  Per-parameter state is ``step`` (a CPU scalar tensor, as
    torch.optim.Adam keeps it), ``exp_avg``, ``exp_avg_sq``: state dicts load into torch.optim.Adam and back.
    ``step`` counts the calls in which the parameter had a gradient, masked or not.

    backend="hip": CUDA/ROCm, float32, contiguous parameters on one device; no fallback.  Not covered: amsgrad, weight
    decay, maximize, sparse gradients, float16 parameters, graph capture."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-15, backend="hip"):
        if backend not in ("hip", "torch"):
            raise ValueError("Invalid backend")
        if not isinstance(params, dict) or not params:
            raise ValueError("GaussianAdam takes a non-empty dict {name: parameter tensor}")
        names = list(params)
        if isinstance(lr, dict):
            missing, unknown = [n for n in names if n not in lr], [n for n in lr if n not in params]
            if missing or unknown:
                raise ValueError(f"lr must cover every parameter name: missing {missing}, unknown {unknown}")
            lrs = {n: float(lr[n]) for n in names}
        else:
            lrs = {n: float(lr) for n in names}
        b1, b2 = (float(b) for b in betas)
        for n in names:
            _check_hyper(lrs[n], b1, b2, float(eps))
            if not isinstance(params[n], torch.Tensor):
                raise ValueError(f"parameter {n!r} is not a tensor")
        self.backend = backend
        self._names = names
        if backend == "hip":
            _check_hip_params([(n, params[n]) for n in names])
        defaults = _adam_flags()
        defaults.update(lr=1e-3 if isinstance(lr, dict) else float(lr), betas=(b1, b2), eps=float(eps))
        super().__init__([{"params": [params[n]], "name": n, "lr": lrs[n]} for n in names], defaults)

    # ------------------------------------------------------------------ groups by name
    def group(self, name):
        for g in self.param_groups:
            if g.get("name") == name:
                return g
        raise ValueError(f"no parameter group named {name!r} (have {[g.get('name') for g in self.param_groups]})")

    def load_state_dict(self, state_dict):
        """As torch's; groups loaded from a torch.optim.Adam keep this optimiser's names, a ``step`` that arrives on a
        device (a fused or capturable Adam's) comes back to the host: the step count is the host's."""
        super().load_state_dict(state_dict)
        for g, n in zip(self.param_groups, self._names):
            g.setdefault("name", n)
        for st in self.state.values():
            if isinstance(st.get("step"), torch.Tensor) and st["step"].device.type != "cpu":
                st["step"] = st["step"].cpu()

    # ------------------------------------------------------------------ the step
    def _work(self, visibility):
        """-> [(p, grad, state, lr, beta1, beta2, eps, t)] of the parameters that have a gradient; their step advanced."""
        work = []
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("weight_decay") or g.get("maximize"):
                raise ValueError("GaussianAdam: amsgrad, weight_decay and maximize are not supported")
            (b1, b2), lr, eps = g["betas"], g["lr"], g["eps"]
            if isinstance(lr, torch.Tensor):
                lr = float(lr)
            _check_hyper(lr, b1, b2, eps)
            for p in g["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise ValueError("GaussianAdam does not support sparse gradients")
                if p.grad.shape != p.shape:
                    raise ValueError(f"{g.get('name')}: gradient {tuple(p.grad.shape)} against parameter {tuple(p.shape)}")
                if visibility is not None and visibility.device != p.device:
                    raise ValueError(f"visibility is on {visibility.device}, {g.get('name')} on {p.device}")
                if visibility is not None and (p.dim() == 0 or p.shape[0] != visibility.shape[0]):
                    raise ValueError(f"{g.get('name')}: shape {tuple(p.shape)} against a visibility mask of "
                                     f"{visibility.shape[0]} rows (a tensor that is not per Gaussian, such as a pose, "
                                     "belongs in its own optimiser)")
                work.append((p, g, float(lr), float(b1), float(b2), float(eps)))
        if work and self.backend == "hip":
            _check_hip_params([(g.get("name"), p) for p, g, *_ in work], [p.grad for p, *_ in work])
        out = []
        for p, g, lr, b1, b2, eps in work:         # (nothing has been changed before every check has passed)
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            out.append((p, p.grad, st, lr, b1, b2, eps, int(st["step"])))
        return out

    @torch.no_grad()
    def step(self, closure=None, *, visibility=None):
        """One update of every parameter that has a gradient.  visibility: None (dense) or a (N,) bool / uint8 tensor on
        the parameters' device: rows where it is zero keep parameter and moments bit for bit (every parameter then needs
        N rows)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if visibility is not None:
            if not isinstance(visibility, torch.Tensor) or visibility.dim() != 1 or visibility.dtype not in (torch.bool, torch.uint8):
                raise ValueError("visibility must be a (N,) bool or uint8 tensor")
        if self.backend == "hip":
            from . import _hip
            _hip.require_cuda(visibility, what="visibility mask")
            _hip.lib()                                  # (a missing library or GPU is an error before anything moves)
        work = self._work(visibility)
        if not work:
            return loss
        if self.backend == "torch":
            for p, grad, st, lr, b1, b2, eps, t in work:
                vis = None if visibility is None else visibility != 0
                adam_update_torch(p, grad, st["exp_avg"], st["exp_avg_sq"], lr, b1, b2, eps, t, vis)
        else:
            self._step_hip(work, visibility)
        return loss

    def _step_hip(self, work, visibility):
        from . import _hip
        dev = work[0][0].device
        vis_ptr, vis_rows, vis = None, 0, None
        if visibility is not None:
            vis = visibility.contiguous()
            vis = vis.view(torch.uint8) if vis.dtype == torch.bool else vis     # (a bool tensor stores bytes 0 / 1)
            vis_ptr, vis_rows = _hip.ptr(vis), vis.numel()
        L = _hip.lib()
        with _hip.on_device(dev):
            stream = _hip.stream(dev)
            for c0 in range(0, len(work), _hip.ADAM_MAX_TENSORS):
                chunk = work[c0:c0 + _hip.ADAM_MAX_TENSORS]
                if any(w[0].numel() == 0 for w in chunk):
                    chunk = [w for w in chunk if w[0].numel()]
                    if not chunk:
                        continue
                table = (_hip.AdamTensor * len(chunk))()
                grads = []                                      # (keeps converted gradients alive until the launch is enqueued)
                for rec, (p, grad, st, lr, b1, b2, eps, t) in zip(table, chunk):
                    g32 = _hip.f32c(grad)
                    grads.append(g32)
                    for k in ("exp_avg", "exp_avg_sq"):         # (a loaded state dict's moments: the parameter's layout)
                        if st[k].dtype != torch.float32 or not st[k].is_contiguous():
                            st[k] = _hip.f32c(st[k])
                    rows = p.shape[0] if p.dim() else 1
                    rec.param, rec.grad = p.data_ptr(), g32.data_ptr()
                    rec.exp_avg, rec.exp_avg_sq = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                    rec.rows, rec.width = rows, p.numel() // rows
                    rec.lr, rec.beta1, rec.beta2, rec.eps = lr, b1, b2, eps
                    rec.bias_correction1, rec.bias_correction2_sqrt = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
                _hip.check(L.ms_adam_step(len(chunk), table, vis_ptr, vis_rows, stream), "ms_adam_step")
        # the kernel wrote through raw pointers: the version counters move as adam_update_torch's three copy_ move them (masked
        # or not, and for a tensor without elements too), so the scene caches and autograd's saved-tensor check see the step
        _hip.bump(*[t for p, _, st, *_ in work for t in (p, st["exp_avg"], st["exp_avg_sq"])])

    # ------------------------------------------------------------------ densification
    def _rows(self, keep, n_old, device):
        if not isinstance(keep, torch.Tensor) or keep.dim() != 1:
            raise ValueError("keep must be a 1-D index tensor or boolean mask")
        if keep.dtype == torch.bool:
            if keep.numel() != n_old:
                raise ValueError(f"keep is a mask of {keep.numel()} rows, the parameters have {n_old}")
            return keep.to(device), int(keep.sum())
        if keep.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"keep must be boolean or an integer index tensor, got {keep.dtype}")
        return keep.to(device=device, dtype=torch.int64), keep.numel()

    @torch.no_grad()
    def relocate(self, new_params, keep, n_new):
        """After a densification: group ``name``'s parameter becomes ``new_params[name]`` (count(keep) + n_new rows) and its
        moments ``cat(old[keep], zeros(n_new, ...))`` -- the order of ``DensifyStats.select(keep).append(n_new)``.
        keep: an index tensor (repeats allowed) or a boolean mask over the old rows.  ``step`` is kept."""
        n_new = int(n_new)
        names = [g.get("name") for g in self.param_groups]
        if not isinstance(new_params, dict):
            raise ValueError("new_params must be a dict {name: tensor}")
        missing, unknown = [n for n in names if n not in new_params], [n for n in new_params if n not in names]
        if missing or unknown or n_new < 0:
            raise ValueError(f"relocate: new_params must name every group exactly: missing {missing}, unknown {unknown}"
                             if missing or unknown else "relocate: n_new is negative")
        plan = []
        for g in self.param_groups:
            (old,), new = g["params"], new_params[g["name"]]
            if not isinstance(new, torch.Tensor) or not new.is_leaf:
                raise ValueError(f"{g['name']}: the new parameter must be a leaf tensor")
            idx, n_keep = self._rows(keep, old.shape[0], old.device)
            if new.shape[0] != n_keep + n_new or new.shape[1:] != old.shape[1:]:
                raise ValueError(f"{g['name']}: the new parameter has shape {tuple(new.shape)}, expected "
                                 f"{(n_keep + n_new, *old.shape[1:])} ({n_keep} kept + {n_new} new rows)")
            if new.dtype != old.dtype or new.device != old.device:
                raise ValueError(f"{g['name']}: the new parameter is {new.dtype} on {new.device}, the old one {old.dtype} on {old.device}")
            plan.append((g, old, new, idx))
        if self.backend == "hip":
            _check_hip_params([(g["name"], new) for g, _, new, _ in plan])
        for g, old, new, idx in plan:
            st = self.state.pop(old, None)
            g["params"] = [new]
            if st:
                for k in ("exp_avg", "exp_avg_sq"):
                    z = torch.zeros((n_new, *old.shape[1:]), dtype=st[k].dtype, device=st[k].device)
                    st[k] = torch.cat([st[k][idx], z]).contiguous()
                self.state[new] = st

    def _adopt(self, new_params, new_moments):
        """relocate's hand-over with ready-made moments (refine.py, backend="hip", which has checked everything): group
        ``name``'s parameter becomes ``new_params[name]``, its moments ``new_moments[name] = [exp_avg, exp_avg_sq]``; a
        parameter without state stays without.  ``step`` is kept."""
        for g in self.param_groups:
            (old,), new = g["params"], new_params[g["name"]]
            st = self.state.pop(old, None)
            g["params"] = [new]
            if st:
                st["exp_avg"], st["exp_avg_sq"] = new_moments[g["name"]]
                self.state[new] = st

    @torch.no_grad()
    def zero_state(self, name):
        """Zero the moments of group ``name`` (3DGS's opacity reset); ``step`` is kept."""
        for p in self.group(name)["params"]:
            st = self.state.get(p)
            if st:
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()


def _check_hyper(lr, b1, b2, eps):
    if not (math.isfinite(lr) and lr >= 0.0):
        raise ValueError(f"Invalid learning rate: {lr}")
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"Invalid betas: ({b1}, {b2}), each must lie in [0, 1)")
    if not eps > 0.0:
        raise ValueError(f"Invalid epsilon value: {eps}")


def _check_hip_params(named, grads=None):
    """ValueError unless every parameter (and gradient) can go to ms_adam_step as it is."""
    from . import _hip
    _hip.require_cuda(*[p for _, p in named], what="parameter")
    if grads:
        _hip.require_cuda(*grads, what="gradient")
    dev = named[0][1].device
    for name, p in named:
        what = f"parameter {name!r}" if name else "every parameter"
        if p.dtype != torch.float32:
            raise ValueError(f"backend='hip': {what} must be float32, got {p.dtype}")
        if not p.is_contiguous():
            raise ValueError(f"backend='hip': {what} must be contiguous")
        if p.device != dev:
            raise ValueError(f"backend='hip': parameters on {p.device} and {dev}; one optimiser, one device")
    for g in grads or ():
        if g.device != dev:
            raise ValueError(f"backend='hip': a gradient on {g.device}, its parameter on {dev}")


__all__ = ["GaussianAdam", "adam_update_torch"]
