"""CPU: GaussianAdam's definition (mojosplat_amd/optim.py, backend="torch") against torch.optim.Adam, its state dicts in
both directions, the semantics of a visibility mask, relocate / zero_state, every ValueError, and the host logic of
ms_adam_step (argument validation needs no GPU)."""
import copy
import ctypes

import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import GaussianAdam, _hip
from mojosplat_amd.densify import DensifyStats

N = 300
SHAPES = {"means3d": (N, 3), "scales": (N, 3), "quats": (N, 4), "opacities": (N,), "features": (N, 16, 3), "rgb": (N, 3)}
LRS = {"means3d": 1.6e-4, "scales": 5e-3, "quats": 1e-3, "opacities": 5e-2, "features": 2.5e-3, "rgb": 1e-2}
REL = 1e-12


def _params(dtype=torch.float64, seed=0, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(s, generator=g, dtype=dtype).requires_grad_(True) for k, s in shapes.items()}


def _set_grads(params, seed, zero_rows=None):
    g = torch.Generator().manual_seed(1000 + seed)
    for p in params.values():
        p.grad = torch.randn(p.shape, generator=g, dtype=p.dtype) * 0.1
        if zero_rows is not None:
            p.grad[zero_rows] = 0


def _close(a, b, what):
    err, ref = float((a - b).abs().max()), float(b.abs().max())
    assert err <= REL * max(ref, 1e-300), f"{what}: max err {err:.3g} against max {ref:.3g}"


def _pair(backend="torch"):
    ours = _params()
    theirs = {k: v.detach().clone().requires_grad_(True) for k, v in ours.items()}
    opt = GaussianAdam(ours, lr=LRS, betas=(0.9, 0.999), eps=1e-15, backend=backend)
    ref = torch.optim.Adam([{"params": [theirs[k]], "lr": LRS[k]} for k in theirs], betas=(0.9, 0.999), eps=1e-15, foreach=False)
    return ours, theirs, opt, ref


def _both_step(ours, theirs, opt, ref, seed):
    _set_grads(ours, seed)
    for k in ours:
        theirs[k].grad = ours[k].grad.clone()
    opt.step()
    ref.step()


def _compare(ours, theirs, opt, ref, what):
    for k in ours:
        _close(ours[k].detach(), theirs[k].detach(), f"{what} {k}")
        for key in ("exp_avg", "exp_avg_sq"):
            _close(opt.state[ours[k]][key], ref.state[theirs[k]][key], f"{what} {k}.{key}")
        assert int(opt.state[ours[k]]["step"]) == int(ref.state[theirs[k]]["step"])


def test_torch_backend_equals_torch_adam_over_25_scheduled_steps():
    ours, theirs, opt, ref = _pair()
    assert [g["name"] for g in opt.param_groups] == list(SHAPES) and [g["lr"] for g in opt.param_groups] == list(LRS.values())
    s1, s2 = torch.optim.lr_scheduler.ExponentialLR(opt, 0.9), torch.optim.lr_scheduler.ExponentialLR(ref, 0.9)
    for it in range(25):
        _both_step(ours, theirs, opt, ref, it)
        s1.step()
        s2.step()
    assert opt.param_groups[0]["lr"] == pytest.approx(1.6e-4 * 0.9 ** 25)
    _compare(ours, theirs, opt, ref, "25 steps")
    opt.zero_grad()
    assert all(p.grad is None for p in ours.values())
    # a float lr covers every group; a parameter without a gradient is skipped and its step does not advance
    a = _params(seed=3)
    o = GaussianAdam(a, lr=0.01, backend="torch")
    assert all(g["lr"] == 0.01 and g["eps"] == 1e-15 for g in o.param_groups)
    _set_grads(a, 0)
    a["quats"].grad = None
    before = a["quats"].detach().clone()
    o.step()
    assert a["quats"] not in o.state and torch.equal(a["quats"].detach(), before)
    assert int(o.state[a["scales"]]["step"]) == 1


def test_state_dicts_load_in_both_directions():
    ours, theirs, opt, ref = _pair()
    for it in range(3):
        _both_step(ours, theirs, opt, ref, it)
    # ours -> torch.optim.Adam
    ours2, theirs2, opt2, ref2 = _pair()
    for k in ours:
        theirs2[k].data.copy_(ours[k].data)
        ours2[k].data.copy_(theirs[k].data)
    ref2.load_state_dict(copy.deepcopy(opt.state_dict()))
    opt2.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert [g["name"] for g in opt2.param_groups] == list(SHAPES)
    for it in range(3, 5):
        _set_grads(ours, it)
        for k in ours:
            for other in (theirs, ours2, theirs2):
                other[k].grad = ours[k].grad.clone()
        for o in (opt, ref, opt2, ref2):
            o.step()
    _compare(ours, theirs2, opt, ref2, "ours -> Adam")
    _compare(ours2, theirs, opt2, ref, "Adam -> ours")
    assert int(opt2.state[ours2["scales"]]["step"]) == 5 and opt2.state[ours2["scales"]]["step"].device.type == "cpu"
    # ours -> ours
    ours3, _, opt3, _ = _pair()
    opt3.load_state_dict(copy.deepcopy(opt.state_dict()))
    for k in ours:
        assert torch.equal(opt3.state[ours3[k]]["exp_avg"], opt.state[ours[k]]["exp_avg"])
    sd = ref.state_dict()
    sd["param_groups"][0]["amsgrad"] = True
    opt3.load_state_dict(sd)
    _set_grads(ours3, 9)
    with pytest.raises(ValueError, match="amsgrad"):
        opt3.step()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_mask_semantics(dtype):
    def fresh():
        p = _params(dtype=dtype, seed=5)
        o = GaussianAdam(p, lr=LRS, backend="torch")
        for it in range(2):                    # non-trivial moments
            _set_grads(p, it)
            o.step()
        _set_grads(p, 7)
        return p, o

    snap = lambda p, o: {k: (p[k].detach().clone(), o.state[p[k]]["exp_avg"].clone(), o.state[p[k]]["exp_avg_sq"].clone())
                         for k in p}
    g = torch.Generator().manual_seed(2)
    mask = torch.rand(N, generator=g) < 0.4
    pd, od = fresh()
    od.step()
    dense = snap(pd, od)
    pm, om = fresh()
    before = snap(pm, om)
    om.step(visibility=mask)
    masked = snap(pm, om)
    pa, oa = fresh()
    oa.step(visibility=torch.ones(N, dtype=torch.uint8))
    alltrue = snap(pa, oa)
    for k in SHAPES:
        for i in range(3):
            assert torch.equal(masked[k][i][~mask], before[k][i][~mask]), f"{k}[{i}]: a masked row changed"
            assert torch.equal(masked[k][i][mask], dense[k][i][mask]), f"{k}[{i}]: a visible row differs from the dense step"
            assert not torch.equal(masked[k][i][mask], before[k][i][mask])
            assert torch.equal(alltrue[k][i], dense[k][i])
        assert int(om.state[pm[k]]["step"]) == 3      # step counts calls, masked or not
    # nothing visible: nothing moves, the count still advances
    pn, on = fresh()
    before = snap(pn, on)
    on.step(visibility=torch.zeros(N, dtype=torch.bool))
    after = snap(pn, on)
    assert all(torch.equal(after[k][i], before[k][i]) for k in SHAPES for i in range(3))
    assert int(on.state[pn["rgb"]]["step"]) == 3


@pytest.mark.parametrize("kind", ["bool", "index"])
def test_relocate_and_zero_state(kind):
    p = _params(seed=8)
    opt = GaussianAdam(p, lr=LRS, backend="torch")
    for it in range(4):
        _set_grads(p, it)
        opt.step()
    g = torch.Generator().manual_seed(3)
    n_new = 17
    if kind == "bool":
        keep = torch.rand(N, generator=g) < 0.9
        n_keep = int(keep.sum())
    else:
        keep = torch.randint(0, N, (N + 40,), generator=g)          # clones: repeated rows
        n_keep = keep.numel()
    old = {k: (opt.state[p[k]]["exp_avg"].clone(), opt.state[p[k]]["exp_avg_sq"].clone()) for k in p}
    new = {k: torch.cat([p[k].detach()[keep], torch.randn((n_new, *p[k].shape[1:]), generator=g, dtype=torch.float64)])
           .requires_grad_(True) for k in p}
    stats = DensifyStats(N).select(keep).append(n_new)
    opt.relocate(new, keep, n_new)
    assert stats.n == n_keep + n_new
    for k in p:
        grp = opt.group(k)
        assert grp["params"][0] is new[k] and p[k] not in opt.state
        st = opt.state[new[k]]
        assert int(st["step"]) == 4
        for i, key in enumerate(("exp_avg", "exp_avg_sq")):
            expect = torch.cat([old[k][i][keep], torch.zeros((n_new, *p[k].shape[1:]), dtype=torch.float64)])
            assert torch.equal(st[key], expect) and st[key].is_contiguous()
            assert st[key].shape == new[k].shape == (stats.n, *p[k].shape[1:])
    # and it goes on stepping: the next step is Adam's fifth on the moved moments
    _set_grads(new, 11)
    m_before = opt.state[new["rgb"]]["exp_avg"].clone()
    opt.step()
    assert int(opt.state[new["rgb"]]["step"]) == 5
    _close(opt.state[new["rgb"]]["exp_avg"], 0.9 * m_before + 0.1 * new["rgb"].grad, "exp_avg after relocate")
    opt.zero_state("opacities")
    st = opt.state[new["opacities"]]
    assert int(st["step"]) == 5 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert opt.state[new["rgb"]]["exp_avg"].any()
    with pytest.raises(ValueError, match="no parameter group"):
        opt.zero_state("colours")
    # a state-less optimiser relocates too (nothing to move)
    q = _params(seed=9)
    o2 = GaussianAdam(q, lr=0.1, backend="torch")
    o2.relocate({k: v.detach()[:10].clone().requires_grad_(True) for k, v in q.items()}, torch.arange(10), 0)
    assert len(o2.state) == 0 and o2.group("rgb")["params"][0].shape[0] == 10


def test_every_value_error():
    p = _params(dtype=torch.float32)
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        GaussianAdam(p, lr=LRS, backend="hip")
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        GaussianAdam(p, lr=LRS)                       # "hip" is the default
    with pytest.raises(ValueError, match="Invalid backend"):
        GaussianAdam(p, lr=LRS, backend="triton")
    with pytest.raises(ValueError, match="missing \\['rgb'\\]"):
        GaussianAdam(p, lr={k: v for k, v in LRS.items() if k != "rgb"}, backend="torch")
    with pytest.raises(ValueError, match="unknown \\['pose'\\]"):
        GaussianAdam(p, lr={**LRS, "pose": 1.0}, backend="torch")
    with pytest.raises(ValueError, match="dict"):
        GaussianAdam(list(p.values()), backend="torch")
    with pytest.raises(ValueError, match="learning rate"):
        GaussianAdam(p, lr=-1.0, backend="torch")
    with pytest.raises(ValueError, match="betas"):
        GaussianAdam(p, lr=0.1, betas=(0.9, 1.0), backend="torch")
    with pytest.raises(ValueError, match="epsilon"):
        GaussianAdam(p, lr=0.1, eps=0.0, backend="torch")
    opt = GaussianAdam(p, lr=LRS, backend="torch")
    _set_grads(p, 0)
    with pytest.raises(ValueError, match="visibility mask of 299 rows"):
        opt.step(visibility=torch.ones(N - 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool or uint8"):
        opt.step(visibility=torch.ones(N))
    with pytest.raises(ValueError, match="bool or uint8"):
        opt.step(visibility=torch.ones(N, 1, dtype=torch.bool))
    assert len(opt.state) == 0                        # a refused step changes nothing
    # a pose next to the Gaussians: fine dense, refused under a mask
    pose = {"rgb": p["rgb"], "pose": torch.zeros(6, requires_grad=True)}
    o2 = GaussianAdam(pose, lr=0.1, backend="torch")
    pose["pose"].grad = torch.ones(6)
    o2.step()
    with pytest.raises(ValueError, match="own optimiser"):
        o2.step(visibility=torch.ones(N, dtype=torch.bool))
    # relocate
    keep = torch.arange(N - 30)
    good = {k: v.detach()[: N - 30 + 5].clone().requires_grad_(True) for k, v in p.items()}
    with pytest.raises(ValueError, match="missing \\['rgb'\\]"):
        opt.relocate({k: v for k, v in good.items() if k != "rgb"}, keep, 5)
    with pytest.raises(ValueError, match="unknown \\['pose'\\]"):
        opt.relocate({**good, "pose": torch.zeros(6, requires_grad=True)}, keep, 5)
    with pytest.raises(ValueError, match="270 kept \\+ 6 new rows"):
        opt.relocate(good, keep, 6)
    with pytest.raises(ValueError, match="mask of 10 rows"):
        opt.relocate(good, torch.ones(10, dtype=torch.bool), 5)
    with pytest.raises(ValueError, match="expected"):
        opt.relocate({**good, "features": good["features"].detach()[:, :4].clone().requires_grad_(True)}, keep, 5)
    assert opt.group("rgb")["params"][0] is p["rgb"]  # a refused relocate changes nothing
    opt.relocate(good, keep, 5)
    assert opt.group("rgb")["params"][0] is good["rgb"]
    assert "GaussianAdam" in ms.__all__ and ms.GaussianAdam is GaussianAdam


def _record(P, **kw):
    f = dict(param=P, grad=P, exp_avg=P, exp_avg_sq=P, rows=100, width=3, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15,
             bias_correction1=0.1, bias_correction2_sqrt=0.0316)
    f.update(kw)
    return _hip.AdamTensor(**f)


def test_library_exports_and_validates_adam_step():
    lib = _hip.load()
    assert hasattr(lib, "ms_adam_step") and "ms_adam_step" in _hip.EXPORTS
    assert lib.ms_version() == 5 == _hip.ABI_VERSION
    P = 0x1000                                         # validation never dereferences it
    INVALID, TOO_LARGE = 1, 3
    err = lambda: lib.ms_last_error_string().decode()

    def call(n=1, vis=None, vis_rows=0, recs=None, **kw):
        recs = recs if recs is not None else [_record(P, **kw)]
        table = (_hip.AdamTensor * max(len(recs), 1))(*recs)
        return lib.ms_adam_step(n, table, vis, vis_rows, None)

    assert call(n=0) == INVALID and "n_tensors" in err()
    assert call(n=9, recs=[_record(P)] * 9) == INVALID and "n_tensors" in err()
    assert lib.ms_adam_step(1, None, None, 0, None) == INVALID and "null" in err()
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert call(**{field: None}) == INVALID and "null" in err()
    assert call(rows=0) == INVALID and "size" in err()
    assert call(width=-3) == INVALID and "size" in err()
    for lr in (-1e-3, float("inf"), float("nan")):
        assert call(lr=lr) == INVALID and "lr" in err()
    for field in ("beta1", "beta2"):
        for b in (1.0, -0.1, float("nan")):
            assert call(**{field: b}) == INVALID and "beta" in err()
    for eps in (0.0, -1e-8, float("nan")):
        assert call(eps=eps) == INVALID and "eps" in err()
    for field in ("bias_correction1", "bias_correction2_sqrt"):
        for b in (0.0, 1.5, -0.5, float("nan")):
            assert call(**{field: b}) == INVALID and "bias correction" in err()
    V = ctypes.c_void_p(0x2000)
    assert call(vis=V, vis_rows=99) == INVALID and "100 rows" in err() and "mask 99" in err()
    assert call(n=2, vis=V, vis_rows=100, recs=[_record(P), _record(P, rows=7)]) == INVALID and "tensor 1" in err()
    assert call(rows=1 << 29, width=4) == TOO_LARGE and "2^31" in err()
    assert call(rows=1 << 31, width=1) == TOO_LARGE and "2^31" in err()
    assert call(rows=1, width=1 << 40) == TOO_LARGE and "2^31" in err()
