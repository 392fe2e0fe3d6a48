"""CPU: the densification step's definition (mojosplat_amd/refine.py, backend="torch"): a hand-worked scene, the literal
"duplicate, then split, then prune" sequence of gsplat's default strategy restated here, the rules that can be switched
off, both opacity spaces, the optimiser's moments against ``relocate``, the noise, every ValueError, ``reset_opacities``,
and the host logic of ms_densify_classify / ms_densify_move (argument validation needs no GPU)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import DensifyStats, GaussianAdam, _hip, densify_and_prune, reset_opacities
from mojosplat_amd.refine import LOG16, _thresholds, child_means_torch

DEFAULTS = dict(grow_grad2d=2e-4, grow_scale3d=0.01, grow_scale2d=0.05, prune_opa=0.005, prune_scale3d=0.1, prune_scale2d=0.15,
                scene_scale=1.0)
WIDTHS = {"means3d": (3,), "scales": (3,), "quats": (4,), "opacities": (), "features": (16, 3), "extra": (5,)}


def make_scene(N, seed, widths=WIDTHS, logit=False):
    """A random float32 scene of N rows and its statistics, with every decision well populated: about a third of the rows
    have a high gradient, scales straddle both scale thresholds, radii both radius thresholds, a sixth is transparent."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    p = {k: torch.randn((N, *w), generator=g) for k, w in widths.items()}
    p["scales"] = (-6.5 + 4.8 * r(N, 1)) - torch.cat([torch.zeros(N, 1), r(N, 2)], 1)[:, torch.randperm(3, generator=g)]
    opa = r(N) ** 3 * 0.999 + 1e-6
    p["opacities"] = (torch.log(opa / (1 - opa)) if logit else opa).reshape(p["opacities"].shape)
    stats = DensifyStats(N)
    stats.count[:] = torch.randint(0, 5, (N,), generator=g).float()
    stats.grad2d[:] = torch.where(r(N) < 0.35, 3e-4 + 3e-4 * r(N), 1.5e-4 * r(N)) * stats.count
    stats.max_radii[:] = 0.2 * r(N) ** 4
    noise = torch.randn((2, N, 3), generator=g)
    return p, stats, noise


def flags(p, stats, thr):
    """The five decision flags of the issue's table, written out once more (float32)."""
    smax = p["scales"].max(-1).values
    g = stats.grad2d / stats.count.clamp_min(1)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    high, small = g > f32(thr["grow_grad2d"]), smax <= f32(thr["log_grow"])
    clone = high & small
    split = (high & ~small) | (stats.max_radii > f32(thr["grow_radius"]))
    lowop = p["opacities"].reshape(-1) < f32(thr["thr_opa"])
    big = (smax > f32(thr["log_big"])) | (stats.max_radii > f32(thr["prune_radius"]))
    childbig = ((smax - f32(LOG16)) > f32(thr["log_big"])) | (stats.max_radii > f32(thr["prune_radius"]))
    return clone, split, lowop, big, childbig


def literal_duplicate_split_prune(p, stats, noise, thr):
    """gsplat's default strategy, step by step on materialised tensors: duplicate (clones appended), split (the rows that
    are not split, clones included, then both sets of samples), prune (on the rows as they now are; a new row carries its
    parent's radius).  -> (rows {name: tensor}, source)."""
    N = p["means3d"].shape[0]
    clone, split, _, _, _ = flags(p, stats, thr)
    idx = torch.arange(N)
    # duplicate
    rows = {k: torch.cat([v, v[clone]]) for k, v in p.items()}
    source = torch.cat([idx, idx[clone]])
    # split: decided on the rows that existed before the duplication
    sel = torch.cat([split, torch.zeros(int(clone.sum()), dtype=torch.bool)])
    out = {}
    for k, v in rows.items():
        kids = [v[sel], v[sel]]
        if k == "scales":
            kids = [v[sel] - torch.tensor(LOG16, dtype=torch.float32)] * 2
        if k == "means3d":
            kids = [child_means_torch(v[sel], rows["scales"][sel], rows["quats"][sel], noise[c][source[sel]]) for c in range(2)]
        out[k] = torch.cat([v[~sel]] + kids)
    source = torch.cat([source[~sel], source[sel], source[sel]])
    # prune
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    gone = (out["opacities"].reshape(-1) < f32(thr["thr_opa"])) | (out["scales"].max(-1).values > f32(thr["log_big"])) | \
        (stats.max_radii[source] > f32(thr["prune_radius"]))
    return {k: v[~gone] for k, v in out.items()}, source[~gone]


def _hand_scene():
    #        grad    smax  radius opacity
    rows = [(1e-4, -5.0, 0.01, 0.5),     # 0 keep
            (4e-4, -5.0, 0.01, 0.5),     # 1 clone
            (4e-4, -3.0, 0.01, 0.5),     # 2 split
            (4e-4, -5.0, 0.06, 0.5),     # 3 clone and split at once (small, and wide on screen)
            (1e-4, -5.0, 0.01, 0.001),   # 4 low-opacity original
            (4e-4, -5.0, 0.01, 0.001),   # 5 low-opacity clone: neither the original nor the clone stays
            (1e-4, -2.0, 0.01, 0.5),     # 6 too-big original
            (4e-4, -1.5, 0.01, 0.5),     # 7 a split whose children are too big (-1.5 - log 1.6 > log 0.1)
            (1e-4, -5.0, 0.06, 0.5),     # 8 a split by radius only
            (0.0, -5.0, 0.01, 0.5),      # 9 never seen (count 0): keep
            (4e-4, -2.0, 0.01, 0.5),     # 10 too big itself, split into children that are not (-2 - log 1.6 < log 0.1)
            (1e-4, -5.0, 0.2, 0.5)]      # 11 too wide on screen: split by radius, and the children inherit the radius
    t = torch.tensor(rows, dtype=torch.float32)
    N = len(rows)
    g = torch.Generator().manual_seed(1)
    p = {"means3d": torch.randn((N, 3), generator=g), "scales": t[:, 1:2] - torch.tensor([0.0, 0.5, 1.0]),
         "quats": torch.randn((N, 4), generator=g), "opacities": t[:, 3].clone(), "features": torch.randn((N, 16, 3), generator=g)}
    stats = DensifyStats(N)
    stats.count[:] = torch.tensor([2.0] * 9 + [0.0] + [3.0] * 2)
    stats.grad2d[:] = t[:, 0] * stats.count
    stats.max_radii[:] = t[:, 2]
    return p, stats, torch.randn((2, N, 3), generator=g)


def test_hand_worked_scene():
    p, stats, noise = _hand_scene()
    res = densify_and_prune(p, stats, noise=noise, backend="torch")
    assert (res.n_kept, res.n_cloned, res.n_split, res.n_pruned) == (3, 2, 4, 5)
    assert res.source.dtype == torch.int64 and res.source.tolist() == [0, 1, 9, 1, 3, 2, 3, 8, 10, 2, 3, 8, 10]
    assert res.stats.n == 13 and not any(t.any() for t in (res.stats.grad2d, res.stats.count, res.stats.max_radii))
    src = res.source
    for k in p:
        assert res.params[k].shape == (13, *p[k].shape[1:]) and res.params[k].is_leaf and not res.params[k].requires_grad
        assert torch.equal(res.params[k][:5], p[k][src[:5]]), f"{k}: an original or a clone is not a bit copy"
        if k not in ("means3d", "scales"):
            assert torch.equal(res.params[k][5:], p[k][src[5:]]), f"{k}: a child's row is not a bit copy"
    assert torch.equal(res.params["scales"][5:], p["scales"][src[5:]] - torch.tensor(LOG16, dtype=torch.float32))
    assert LOG16 == float(np.float32(math.log(1.6)))
    for c in range(2):
        rows = src[5 + 4 * c: 9 + 4 * c]
        want = child_means_torch(p["means3d"][rows].double(), p["scales"][rows].double(), p["quats"][rows].double(), noise[c][rows].double())
        # the formula once more, row by row, in float64 numpy
        for j, i in enumerate(rows.tolist()):
            w, x, y, z = (p["quats"][i].double() / p["quats"][i].double().norm()).tolist()
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                          [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
            m = p["means3d"][i].double().numpy() + R @ (np.exp(p["scales"][i].double().numpy()) * noise[c, i].double().numpy())
            assert np.abs(want[j].numpy() - m).max() <= 1e-14
        got = res.params["means3d"][5 + 4 * c: 9 + 4 * c].double()
        assert float((got - want).abs().max()) <= 16 * torch.finfo(torch.float32).eps * float(want.abs().max())
    assert not torch.equal(res.params["means3d"][5:9], res.params["means3d"][9:13])     # the two children differ
    # requires_grad follows the inputs
    q = {k: v.clone().requires_grad_(k != "quats") for k, v in p.items()}
    r2 = densify_and_prune(q, stats, noise=noise, backend="torch")
    assert all(r2.params[k].is_leaf and r2.params[k].requires_grad == (k != "quats") for k in q)
    assert all(torch.equal(r2.params[k], res.params[k]) for k in p)


@pytest.mark.parametrize("N,seed", [(1, 0), (50, 1), (997, 2), (4000, 3)])
def test_one_pass_equals_duplicate_then_split_then_prune(N, seed):
    p, stats, noise = make_scene(N, seed)
    thr = _thresholds(**DEFAULTS, opacity_space="linear")
    rows, source = literal_duplicate_split_prune(p, stats, noise, thr)
    res = densify_and_prune(p, stats, noise=noise, backend="torch", **DEFAULTS)
    assert torch.equal(res.source, source)
    for k in p:
        assert torch.equal(res.params[k], rows[k]), f"{k}: the one-pass definition differs from the literal sequence"
    clone, split, lowop, big, childbig = flags(p, stats, thr)
    assert res.n_kept == int((~split & ~lowop & ~big).sum()) and res.n_cloned == int((clone & ~lowop & ~big).sum())
    assert res.n_split == int((split & ~lowop & ~childbig).sum())
    assert res.n_pruned == N - len(set(source.tolist())) and res.stats.n == source.numel()
    if N >= 997:
        assert min(res.n_kept, res.n_cloned, res.n_split, res.n_pruned) > 0 and int((clone & split).sum()) > 0


def test_a_rule_passed_as_none_is_off():
    p, stats, noise = make_scene(3000, 5)
    run = lambda **kw: densify_and_prune(p, stats, noise=noise, backend="torch", **{**DEFAULTS, **kw})
    base = run()
    inf = float("inf")
    for rule, huge in (("grow_scale2d", 1e30), ("prune_scale3d", 1e30), ("prune_scale2d", 1e30)):
        off, never = run(**{rule: None}), run(**{rule: huge})
        assert _thresholds(**{**DEFAULTS, rule: None}, opacity_space="linear")[
            {"grow_scale2d": "grow_radius", "prune_scale3d": "log_big", "prune_scale2d": "prune_radius"}[rule]] == inf
        assert torch.equal(off.source, never.source) and not torch.equal(off.source, base.source), rule
    # all three off: what is left is the gradient rule and the opacity rule
    res = run(grow_scale2d=None, prune_scale3d=None, prune_scale2d=None)
    high = stats.mean_grad() > torch.tensor(2e-4, dtype=torch.float32)
    small = p["scales"].max(-1).values <= torch.tensor(math.log(0.01), dtype=torch.float32)
    ok = ~(p["opacities"] < torch.tensor(0.005, dtype=torch.float32))
    idx = torch.arange(3000)
    assert torch.equal(res.source, torch.cat([idx[~(high & ~small) & ok], idx[high & small & ok], idx[high & ~small & ok], idx[high & ~small & ok]]))


def test_both_opacity_spaces_agree_when_the_inputs_correspond():
    p, stats, noise = make_scene(2000, 7)
    q, _, _ = make_scene(2000, 7, logit=True)
    assert torch.equal(q["scales"], p["scales"])
    # (rows whose opacity sits within rounding of the threshold could fall either way: there are none in this scene)
    assert not ((p["opacities"] - 0.005).abs() < 1e-6).any()
    a = densify_and_prune(p, stats, noise=noise, backend="torch")
    b = densify_and_prune(q, stats, noise=noise, backend="torch", opacity_space="logit")
    assert torch.equal(a.source, b.source) and a.n_pruned == b.n_pruned > 0
    assert torch.equal(a.params["means3d"], b.params["means3d"])
    # (N, 1) opacities are taken as (N,) ones
    p1 = dict(p, opacities=p["opacities"].reshape(-1, 1))
    c = densify_and_prune(p1, stats, noise=noise, backend="torch")
    assert torch.equal(c.source, a.source) and c.params["opacities"].shape == (a.source.numel(), 1)


def _stepped(p, steps=2, seed=3):
    p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    opt = GaussianAdam(p, lr=1e-3, backend="torch")
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for v in p.values():
            v.grad = torch.randn(v.shape, generator=g)
        opt.step()
    return p, opt


def test_the_optimiser_follows_as_relocate_would():
    p0, stats, noise = make_scene(1500, 11)
    p, opt = _stepped(p0)
    q, ref = _stepped(p0)
    res = densify_and_prune(p, stats, opt, noise=noise, backend="torch")
    plain = densify_and_prune({k: v.detach() for k, v in q.items()}, stats, noise=noise, backend="torch")
    keep = torch.zeros(1500, dtype=torch.bool)
    keep[plain.source[:plain.n_kept]] = True
    new = {k: v.clone().requires_grad_(True) for k, v in plain.params.items()}
    ref.relocate(new, keep, plain.n_cloned + 2 * plain.n_split)
    for k in p:
        assert opt.group(k)["params"][0] is res.params[k] and p[k] not in opt.state and res.params[k].requires_grad
        st, want = opt.state[res.params[k]], ref.state[new[k]]
        assert int(st["step"]) == 2
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[key], want[key]) and st[key].shape == res.params[k].shape
            assert not st[key][res.n_kept:].any() and st[key][:res.n_kept].any()
    # it goes on stepping
    for v in res.params.values():
        v.grad = torch.ones_like(v)
    opt.step()
    assert int(opt.state[res.params["means3d"]]["step"]) == 3
    # an optimiser that has never stepped: nothing to move, the groups adopt the new tensors
    p2 = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    fresh = GaussianAdam(p2, lr=1e-3, backend="torch")
    r2 = densify_and_prune(p2, stats, fresh, noise=noise, backend="torch")
    assert len(fresh.state) == 0 and all(fresh.group(k)["params"][0] is r2.params[k] for k in p2)
    assert r2.n_split > 0 and r2.params["scales"].shape[0] == r2.source.numel()
    for v in r2.params.values():
        v.grad = torch.ones_like(v)
    fresh.step()
    assert int(fresh.state[r2.params["scales"]]["step"]) == 1


def test_noise_is_reproducible_from_a_generator():
    p, stats, noise = make_scene(500, 13)
    run = lambda seed: densify_and_prune(p, stats, generator=torch.Generator().manual_seed(seed), backend="torch")
    a, b, c = run(4), run(4), run(5)
    assert a.n_split > 0 and all(torch.equal(a.params[k], b.params[k]) for k in p)
    assert torch.equal(a.source, c.source) and not torch.equal(a.params["means3d"], c.params["means3d"])
    first = a.n_kept + a.n_cloned
    assert torch.equal(a.params["means3d"][:first], c.params["means3d"][:first])
    given = densify_and_prune(p, stats, noise=torch.randn((2, 500, 3), generator=torch.Generator().manual_seed(4)), backend="torch")
    assert torch.equal(given.params["means3d"], a.params["means3d"])


def test_every_value_error_and_a_refused_call_changes_nothing():
    p0, stats, noise = make_scene(300, 17)
    p, opt = _stepped(p0)
    before = {k: (v.detach().clone(), opt.state[v]["exp_avg"].clone()) for k, v in p.items()}
    stats_before = [t.clone() for t in (stats.grad2d, stats.count, stats.max_radii)]
    call = lambda params=p, st=stats, o=opt, **kw: densify_and_prune(params, st, o, **{"noise": noise, "backend": "torch", **kw})
    for name in ("means3d", "scales", "quats", "opacities"):
        with pytest.raises(ValueError, match=name):
            call({k: v for k, v in p.items() if k != name}, o=None)
    with pytest.raises(ValueError, match="299 rows"):
        call({**p, "extra": p["extra"].detach()[:299]}, o=None)
    with pytest.raises(ValueError, match="shape"):
        call({**p, "quats": p["means3d"]}, o=None)
    with pytest.raises(ValueError, match="opacities"):
        call({**p, "opacities": torch.rand(300, 2)}, o=None)
    with pytest.raises(ValueError, match="densify.grad2d"):
        call(st=DensifyStats(299))
    with pytest.raises(ValueError, match="DensifyStats"):
        call(st=None)
    for bad in (noise[:1], noise.double(), noise[:, :299], noise.reshape(2, 900), noise.to("meta")):
        with pytest.raises(ValueError, match="noise"):
            call(noise=bad)
    with pytest.raises(ValueError, match="opt's groups"):
        call({k: v for k, v in p.items() if k != "extra"})                 # the optimiser holds a tensor params does not
    with pytest.raises(ValueError, match="opt's groups"):
        call({**p, "more": torch.rand(300, 2)})                            # and the other way round
    with pytest.raises(ValueError, match="opt's groups"):
        call({**p, "extra": p["extra"].detach().clone()})                  # the same names, another tensor
    with pytest.raises(ValueError, match="GaussianAdam"):
        call(o=torch.optim.Adam(list(p.values())))
    with pytest.raises(ValueError, match="opacity_space"):
        call(opacity_space="sigmoid")
    with pytest.raises(ValueError, match="backend"):
        call(backend="triton")
    with pytest.raises(ValueError, match="prune_opa"):
        call(prune_opa=-1.0)
    # backend="hip" (the default) has no fallback: CPU tensors are refused
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        densify_and_prune(p, stats, opt, noise=noise)
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        densify_and_prune(p, stats, noise=noise, backend="hip")
    for k, v in p.items():
        assert opt.group(k)["params"][0] is v and torch.equal(v.detach(), before[k][0]) and torch.equal(opt.state[v]["exp_avg"], before[k][1])
    assert all(torch.equal(a, b) for a, b in zip(stats_before, (stats.grad2d, stats.count, stats.max_radii)))
    assert call().n_split > 0                                               # and the same call, unbroken, goes through


@pytest.mark.parametrize("space", ["linear", "logit"])
def test_reset_opacities_clamps_and_zeroes_the_moments(space):
    p0, _, _ = make_scene(400, 19, logit=space == "logit")
    p, opt = _stepped(p0)
    cap = 0.01 if space == "linear" else math.log(0.01 / 0.99)
    was = p["opacities"].detach().clone()
    assert (was > cap).any() and (was < cap).any()
    out = reset_opacities(p["opacities"], opt, opacity_space=space)
    assert out is p["opacities"] and torch.equal(p["opacities"].detach(), was.clamp(max=cap))
    st = opt.state[p["opacities"]]
    assert int(st["step"]) == 2 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert opt.state[p["scales"]]["exp_avg"].any()
    reset_opacities(p["opacities"], max_opacity=0.001, opacity_space=space)           # without an optimiser
    assert float(p["opacities"].detach().max()) <= (0.001 if space == "linear" else math.log(0.001 / 0.999)) + 1e-6
    with pytest.raises(ValueError, match="no group"):
        reset_opacities(torch.rand(400), opt)
    with pytest.raises(ValueError, match="opacity_space"):
        reset_opacities(p["opacities"], opt, opacity_space="sigmoid")


def test_exports():
    for name in ("densify_and_prune", "reset_opacities", "DensifyResult"):
        assert name in ms.__all__ and hasattr(ms, name)
    assert ms.densify_and_prune is densify_and_prune and ms.DensifyResult is ms.refine.DensifyResult


def test_library_exports_and_validates_the_densify_entry_points():
    lib = _hip.load()
    for name in ("ms_densify_workspace_bytes", "ms_densify_classify", "ms_densify_move"):
        assert hasattr(lib, name) and name in _hip.EXPORTS
    assert lib.ms_version() == 5 == _hip.ABI_VERSION
    assert (_hip.DENSIFY_ROWS, _hip.DENSIFY_SCAN_SPAN, _hip.DENSIFY_MAX_TENSORS) == (256, 512, 16)
    P = ctypes.c_void_p(0x1000)                        # validation never dereferences it
    OK, INVALID, WORKSPACE, TOO_LARGE = 0, 1, 2, 3
    err = lambda: lib.ms_last_error_string().decode()
    rules = _hip.DensifyRules(**_thresholds(**DEFAULTS, opacity_space="linear"))
    BIG = 1 << 40
    assert lib.ms_densify_workspace_bytes(0) == 0 and lib.ms_densify_workspace_bytes(1000) == 1008 + 4 * 4 * 4

    def classify(N=1000, ptrs=(P,) * 5, r=rules, ws=P, ws_bytes=BIG, totals=P):
        return lib.ms_densify_classify(N, *ptrs, ctypes.byref(r) if r is not None else None, ws, ws_bytes, totals, None)

    assert classify(N=-1) == INVALID and "negative" in err()
    assert classify(r=None) == INVALID and "null" in err()
    for i in range(5):
        assert classify(ptrs=tuple(None if j == i else P for j in range(5))) == INVALID and "null" in err()
    assert classify(ws=None) == INVALID and "null" in err()
    assert classify(totals=None) == INVALID and "null" in err()
    assert classify(r=_hip.DensifyRules(**{**_thresholds(**DEFAULTS, opacity_space="linear"), "thr_opa": float("nan")})) == INVALID \
        and "NaN" in err()
    assert classify(ws_bytes=100) == WORKSPACE and "workspace" in err()
    assert classify(N=0, ptrs=(None,) * 5, ws=None, totals=None) == OK
    assert classify(N=(1 << 31) // 3 + 1) == TOO_LARGE and "2^31" in err()

    def move(N=1000, k=900, c=50, s=40, ws=P, ws_bytes=BIG, n=1, recs=None, rows=(None,) * 6, **kw):
        f = dict(src=0x1000, dst=0x2000, width=3, kind=_hip.DENSIFY_COPY)
        f.update(kw)
        recs = recs if recs is not None else [_hip.DensifyTensor(**f)]
        table = (_hip.DensifyTensor * max(len(recs), 1))(*recs)
        return lib.ms_densify_move(N, k, c, s, ws, ws_bytes, n, table, *rows, None)

    for field in ("N", "k", "c", "s"):
        assert move(**{field: -1}) == INVALID and "negative" in err()
    assert move(k=1001) == INVALID and "more kept" in err()
    assert move(n=-1) == INVALID and "n_tensors" in err()
    assert move(n=17, recs=[_hip.DensifyTensor(src=1, dst=1, width=1, kind=0)] * 17) == INVALID and "n_tensors" in err()
    assert move(ws=None) == INVALID and "null" in err()
    assert lib.ms_densify_move(1000, 900, 50, 40, P, BIG, 1, None, *(None,) * 6, None) == INVALID and "null" in err()
    assert move(src=None) == INVALID and "null" in err()
    assert move(dst=None) == INVALID and "null" in err()
    assert move(rows=(P, P, P, None, P, P)) == INVALID and "all or none" in err()
    assert move(n=0) == INVALID and "nothing to move" in err()
    assert move(width=0) == INVALID and "size" in err()
    assert move(width=-4) == INVALID and "size" in err()
    assert move(kind=4) == INVALID and "kind" in err()
    assert move(kind=_hip.DENSIFY_SCALE, width=4) == INVALID and "width 4" in err()
    assert move(ws_bytes=100) == WORKSPACE and "workspace" in err()
    assert move(N=0, k=0, c=0, s=0, ws=None, n=0) == OK
    assert move(k=0, c=0, s=0, ws=None, n=0) == OK                        # no output row: nothing to write
    assert move(width=1 << 22) == TOO_LARGE and "2^31" in err()            # 1000 rows x 2^22
    assert move(N=1 << 20, k=1 << 20, c=1 << 20, s=1 << 20, width=512) == TOO_LARGE and "2^31" in err()   # fits before, not after
    assert move(N=1 << 30, k=5, c=5, s=5) == TOO_LARGE and "2^31" in err()
