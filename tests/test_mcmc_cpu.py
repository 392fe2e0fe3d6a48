"""CPU: the MCMC strategy's definition (mojosplat_amd/mcmc.py, backend="torch"): the relocation formula in float64 against
the literal double sum, the integer sampler's statistics, relocate_dead / grow / inject_noise row by row, the optimiser's
moments, every ValueError, and the host logic of ms_mcmc_sample / ms_mcmc_apply / ms_mcmc_noise (argument validation needs
no GPU)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import GaussianAdam, _hip, grow, inject_noise, relocate_dead
from mojosplat_amd.mcmc import BINOM, dead_and_cum_torch, noise_step_torch, relocated_torch, sample_torch

WIDTHS = {"means3d": (3,), "scales": (3,), "quats": (4,), "opacities": (), "features": (16, 3), "extra": (5,)}
KEYS = ("exp_avg", "exp_avg_sq")


def make_scene(N, seed, widths=WIDTHS, logit=False, dead=0.3):
    """A random float32 scene of N rows; a fraction ``dead`` of the rows (scattered) has opacity 0.001, the rest lies in
    [0.006, 0.99]."""
    g = torch.Generator().manual_seed(seed)
    p = {k: torch.randn((N, *w), generator=g) for k, w in widths.items()}
    p["scales"] = -5.0 + 2.0 * torch.rand((N, 3), generator=g)
    opa = 0.006 + 0.984 * torch.rand(N, generator=g)
    opa[torch.rand(N, generator=g) < dead] = 0.001
    p["opacities"] = (torch.log(opa / (1 - opa)) if logit else opa).reshape(p["opacities"].shape)
    return p


def draws_for(n, seed):
    return torch.rand(n, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def stepped(p, steps=2, seed=3):
    p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    opt = GaussianAdam(p, lr=1e-3, backend="torch")
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for v in p.values():
            v.grad = torch.randn(v.shape, generator=g)
        opt.step()
    for v in p.values():
        v.grad = None
    return p, opt


def literal_D(op, n):
    """The issue's double sum, term by term, in Python floats with exact binomials."""
    return sum(math.comb(a - 1, b) * (-1.0) ** b / math.sqrt(b + 1.0) * op ** (b + 1) for a in range(1, n + 1) for b in range(a))


def test_binomial_table_is_the_inner_sum_carried_out():
    assert BINOM.shape == (51, 51) and BINOM.dtype == torch.float32
    for n in (1, 2, 5, 17, 51):
        for b in range(51):
            want = sum(math.comb(a - 1, b) for a in range(b + 1, n + 1)) * (-1.0) ** b / math.sqrt(b + 1.0)
            assert float(BINOM[n - 1, b]) == float(np.float32(want)), (n, b)


def test_relocation_formula_in_float64():
    o = torch.tensor([0.006, 0.1, 0.5, 0.9, 0.99], dtype=torch.float64)
    one = torch.ones(5, dtype=torch.int64)
    # n = 1: the row keeps its opacity and its scale (D = o)
    o1, dlog1 = relocated_torch(o, one)
    assert float((o1 - o).abs().max()) <= 1e-15 and float(dlog1.abs().max()) <= 1e-15
    for n in (2, 5, 51):
        on, dlog = relocated_torch(o, n * one, min_opacity=1e-9)         # (no clamp: the formula itself)
        coef = dlog.exp()
        assert bool(((coef > 0) & (coef <= 1)).all()), (n, coef)
        # n Gaussians of opacity o' composite to o
        assert float((1 - (1 - on) ** n - o).abs().max()) <= 1e-12
        # the table's sum is the literal double sum (up to the float32 rounding of its coefficients, amplified by the
        # cancellation of the alternating sum: the largest term over the result, times 2^-24)
        for oi, opi, di in zip(o.tolist(), on.tolist(), dlog.tolist()):
            lit = literal_D(opi, n)
            top = max(math.comb(n, b + 1) * opi ** (b + 1) / math.sqrt(b + 1.0) for b in range(n))
            assert abs(oi / math.exp(di) - lit) <= 4 * 2.0 ** -24 * top, (n, oi)
    # a ratio above 51 counts as 51
    a, b = relocated_torch(o, 51 * one), relocated_torch(o, 80 * one)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the clamp
    lo, _ = relocated_torch(o[:1], 51 * one[:1], min_opacity=0.005)
    assert float(lo) == 0.005


def test_sampler_statistics():
    N, n_draws = 4000, 200_000
    g = torch.Generator().manual_seed(0)
    opa = 0.005 + 0.99 * torch.rand(N, generator=g)
    dead, cum = dead_and_cum_torch(opa, 0.005, "linear")
    w = torch.diff(cum, prepend=torch.zeros(1, dtype=torch.int64))
    assert torch.equal(w == 0, dead) and torch.equal(w[~dead], torch.round(opa[~dead] * 2 ** 24).long())
    s = sample_torch(cum, dead, torch.rand(n_draws, dtype=torch.float64, generator=g))
    assert int(s.min()) >= 0 and not dead[s].any(), "a zero-weight row was drawn"
    count = torch.bincount(s, minlength=N).double()
    expected = n_draws * w.double() / float(cum[-1])
    live = ~dead
    chi = float((((count - expected) ** 2 / expected)[live]).mean())
    print(f"\n[mcmc sampler] mean (count - expected)^2 / expected over {int(live.sum())} live rows = {chi:.4f}")
    assert abs(chi - 1.0) <= 0.1
    # both ends of [0, 1): the first and the last live row
    ends = sample_torch(cum, dead, torch.tensor([0.0, 1.0 - 2.0 ** -53], dtype=torch.float64))
    first, last = int(torch.nonzero(live)[0]), int(torch.nonzero(live)[-1])
    assert ends.tolist() == [first, last]
    # logit space: the same rows are dead
    dead2, _ = dead_and_cum_torch(torch.log(opa / (1 - opa)), 0.005, "logit")
    assert int((dead2 != dead).sum()) <= 1          # (a row within rounding of the threshold may fall either way)
    # a NaN is dead
    assert dead_and_cum_torch(torch.tensor([float("nan"), 0.5]), 0.005, "linear")[0].tolist() == [True, False]


@pytest.mark.parametrize("space", ["linear", "logit"])
def test_relocate_dead(space):
    N = 1500
    p0 = make_scene(N, 11, logit=space == "logit")
    p, opt = stepped(p0)
    before = {k: v.detach().clone() for k, v in p.items()}
    m_before = {k: {key: opt.state[v][key].clone() for key in KEYS} for k, v in p.items()}
    dead, cum = dead_and_cum_torch(before["opacities"], 0.005, space)
    u = draws_for(N, 5)
    res = relocate_dead(p, opt, opacity_space=space, draws=u, backend="torch")
    n = int(res.n)
    assert res.params is p and isinstance(res.n, torch.Tensor) and res.n.dtype == torch.int64
    assert res.sampled.dtype == res.targets.dtype == torch.int64 and res.sampled.shape == res.targets.shape == (N,)
    # the targets are exactly the dead rows in ascending order
    assert n == int(dead.sum()) > 100 and torch.equal(res.targets[:n], torch.nonzero(dead).reshape(-1))
    assert (res.targets[n:] == -1).all() and (res.sampled[n:] == -1).all()
    s, t = res.sampled[:n], res.targets[:n]
    assert torch.equal(s, sample_torch(cum, dead, u[:n])) and not dead[s].any()
    touched = torch.zeros(N, dtype=torch.bool)
    touched[s] = True
    touched[t] = True
    counts = torch.bincount(s, minlength=N)
    src = torch.nonzero(counts).reshape(-1)
    for k in p:
        now = p[k].detach()
        assert torch.equal(now[~touched], before[k][~touched]), f"{k}: an untouched row changed"
        if k not in ("opacities", "scales"):
            assert torch.equal(now[~dead], before[k][~dead]), f"{k}: a live row changed"
            assert torch.equal(now[t], before[k][s]), f"{k}: a target is not a bit copy of its source"
        else:
            assert torch.equal(now[t], now[s]), f"{k}: a target does not share its source's new value"
        st = opt.state[p[k]]
        assert int(st["step"]) == 2
        for key in KEYS:
            assert not st[key][touched].any() and torch.equal(st[key][~touched], m_before[k][key][~touched])
            assert st[key][~touched].any()
    # the new values, from the float64 evaluation of the formula
    o = before["opacities"].reshape(-1)[src].double()
    o = torch.sigmoid(o) if space == "logit" else o
    o_new, dlog = relocated_torch(o, counts[src] + 1)
    got_o = p["opacities"].detach().reshape(-1)[src].double()
    got_o = torch.sigmoid(got_o) if space == "logit" else got_o
    assert float(((got_o - o_new) / o_new).abs().max()) <= 1e-5
    want_s = before["scales"][src].double() + dlog.unsqueeze(-1)
    assert float((p["scales"].detach()[src].double() - want_s).abs().max()) <= 1e-5
    assert bool((dlog <= 0).all())
    # every target is at or above the threshold (exactly on it where the clamp caught a source that was drawn often)
    lowest = float(torch.tensor(0.005 if space == "linear" else math.log(0.005 / 0.995), dtype=torch.float32))
    assert float(p["opacities"].detach().reshape(-1)[t].min()) >= lowest - (1e-6 if space == "logit" else 0.0)


def test_relocate_dead_no_ops_and_given_samples():
    N = 300
    p = make_scene(N, 3, dead=0.0)
    before = {k: v.clone() for k, v in p.items()}
    res = relocate_dead(p, opacity_space="linear", draws=draws_for(N, 1), backend="torch")
    assert int(res.n) == 0 and (res.sampled == -1).all() and all(torch.equal(p[k], before[k]) for k in p)
    q = make_scene(N, 3, dead=0.0)
    q["opacities"].fill_(0.001)                             # all dead: total == 0
    q["opacities"][7] = float("nan")
    before = {k: v.clone() for k, v in q.items()}
    res = relocate_dead(q, opacity_space="linear", draws=draws_for(N, 1), backend="torch")
    assert int(res.n) == 0 and (res.targets == -1).all()
    assert all(torch.equal(torch.nan_to_num(q[k]), torch.nan_to_num(before[k])) for k in q)
    # (N, 1) opacities; the caller's own samples; a sample that is dead or out of range is skipped
    r = make_scene(N, 5)
    r["opacities"] = r["opacities"].reshape(N, 1)
    dead, _ = dead_and_cum_torch(r["opacities"], 0.005, "linear")
    live_rows, dead_rows = torch.nonzero(~dead).reshape(-1), torch.nonzero(dead).reshape(-1)
    mine = torch.full((N,), int(live_rows[0]))
    mine[1], mine[2] = int(dead_rows[0]), N + 5
    before = {k: v.clone() for k, v in r.items()}
    res = relocate_dead(r, opacity_space="linear", sampled=mine, backend="torch")
    n = int(res.n)
    assert n == dead_rows.numel() and res.sampled[:3].tolist() == [int(live_rows[0]), -1, -1] and r["opacities"].shape == (N, 1)
    assert torch.equal(r["features"][dead_rows[1]], before["features"][dead_rows[1]])       # skipped: untouched
    assert torch.equal(r["features"][dead_rows[0]], before["features"][live_rows[0]])
    # one source, many targets: the ratio is clamped at 51
    if n - 2 > 51:
        want, _ = relocated_torch(before["opacities"].reshape(-1)[live_rows[:1]].double(), torch.tensor([51]))
        assert abs(float(r["opacities"][live_rows[0]]) - float(want)) <= 1e-6


def test_grow():
    N = 1000
    p0 = make_scene(N, 21)
    p, opt = stepped(p0)
    before = {k: v.detach().clone() for k, v in p.items()}
    m_before = {k: opt.state[v]["exp_avg"].clone() for k, v in p.items()}
    # cap_max <= N: nothing is done
    res = grow(p, opt, cap_max=N, opacity_space="linear", backend="torch")
    assert res.n == 0 and res.params is p and res.sampled.numel() == 0 and opt.group("scales")["params"][0] is p["scales"]
    assert grow(p, opt, cap_max=500, opacity_space="linear", backend="torch").n == 0
    assert grow(p, opt, cap_max=5000, growth=1.0, opacity_space="linear", backend="torch").n == 0
    # the cap binds
    assert grow({k: v.detach() for k, v in p.items()}, cap_max=1020, opacity_space="linear", backend="torch",
                generator=torch.Generator().manual_seed(1)).params["quats"].shape == (1020, 4)
    u = draws_for(50, 9)
    res = grow(p, opt, cap_max=100_000, opacity_space="linear", draws=u, backend="torch")
    assert res.n == 50 == int(1.05 * N) - N and torch.equal(res.targets, torch.arange(N, N + 50))
    dead, cum = dead_and_cum_torch(before["opacities"], 0.005, "linear")
    s = res.sampled
    assert torch.equal(s, sample_torch(cum, dead, u)) and not dead[s].any()
    changed = torch.zeros(N, dtype=torch.bool)
    changed[s] = True
    for k in p:
        new = res.params[k]
        assert new.shape == (N + 50, *p[k].shape[1:]) and new.is_leaf and new.requires_grad
        assert opt.group(k)["params"][0] is new and p[k] not in opt.state
        assert torch.equal(new.detach()[:N][~changed], before[k][~changed])
        assert torch.equal(new.detach()[N:], new.detach()[s]), f"{k}: the appended rows are not in draw order"
        if k not in ("opacities", "scales"):
            assert torch.equal(new.detach()[:N], before[k])
        st = opt.state[new]
        assert int(st["step"]) == 2 and st["exp_avg"].shape == new.shape
        assert not st["exp_avg"][N:].any() and not st["exp_avg"][:N][changed].any()
        assert torch.equal(st["exp_avg"][:N][~changed], m_before[k][~changed])
    assert bool((res.params["scales"].detach()[s] < before["scales"][s]).all())
    snap = {k: v.detach().clone() for k, v in res.params.items()}
    # GaussianAdam steps afterwards
    for v in res.params.values():
        v.grad = torch.ones_like(v)
    opt.step()
    assert int(opt.state[res.params["means3d"]]["step"]) == 3
    # requires_grad follows the inputs; without an optimiser
    q = {k: v.clone().requires_grad_(k != "quats") for k, v in before.items()}
    r2 = grow(q, cap_max=100_000, opacity_space="linear", draws=u, backend="torch")
    assert all(r2.params[k].is_leaf and r2.params[k].requires_grad == (k != "quats") for k in q)
    assert all(torch.equal(r2.params[k].detach(), snap[k]) for k in q)
    # nothing alive: the new rows are copies of row 0, nothing is rewritten
    z = {k: v.clone() for k, v in p0.items()}
    z["opacities"].fill_(0.001)
    r3 = grow(z, cap_max=100_000, opacity_space="linear", draws=u, backend="torch")
    assert (r3.sampled == -1).all() and all(torch.equal(r3.params[k][:N], z[k]) for k in z)
    assert all(torch.equal(r3.params[k][N:], z[k][:1].expand(50, *z[k].shape[1:])) for k in z)


def test_inject_noise():
    N = 64
    g = torch.Generator().manual_seed(2)
    p = make_scene(N, 31, dead=0.0)
    p["opacities"][: N // 2] = 1.0
    p["opacities"][N // 2:] = 0.001
    noise = torch.randn((N, 3), generator=g)
    before = {k: v.clone() for k, v in p.items()}
    lr, noise_lr = 1.6e-4, 5e5
    version = p["means3d"]._version
    assert inject_noise(p, lr, noise_lr=noise_lr, opacity_space="linear", noise=noise, backend="torch") is None
    assert p["means3d"]._version > version
    assert all(torch.equal(p[k], before[k]) for k in p if k != "means3d")
    moved = p["means3d"].double() - before["means3d"].double()
    # float64 evaluation, row by row, in numpy: Sigma @ (noise * gate * lr * noise_lr)
    want = np.zeros((N, 3))
    for i in range(N):
        w, x, y, z = (before["quats"][i].double() / before["quats"][i].double().norm()).tolist()
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        Sigma = R @ np.diag(np.exp(2 * before["scales"][i].double().numpy())) @ R.T
        o = float(before["opacities"][i])
        arg = -100.0 * ((1.0 - o) - 0.995)
        gate = 0.0 if arg > 700 else 1.0 / (1.0 + math.exp(arg))
        want[i] = Sigma @ (noise[i].double().numpy() * gate * lr * noise_lr)
    step = np.abs(want[N // 2:]).max()
    # o = 1: the gate is below 1e-40 of the step (in float32 it is exactly 0)
    assert float(moved[: N // 2].abs().max()) <= 1e-40 * step and np.abs(want[: N // 2]).max() <= 1e-40 * step
    # o = 0.001: the gate is sigmoid(0.4) = 0.599; the row moves by the float64 value within float32 rounding (of the sum
    # mean + step, and of the dozen operations of the step)
    d64 = noise_step_torch(before["scales"].double(), before["quats"].double(), before["opacities"].double(), noise, lr * noise_lr,
                           "linear")
    assert float(np.abs(d64.numpy() - want)[N // 2:].max()) <= 1e-12 * step
    eps = float(torch.finfo(torch.float32).eps)
    err = (moved[N // 2:].numpy() - want[N // 2:])
    bound = eps * before["means3d"][N // 2:].abs().double().numpy() + 16 * eps * np.abs(want[N // 2:]).max(-1, keepdims=True)
    assert (np.abs(err) <= bound).all() and step > 1e-6
    # logit space, drawn noise, reproducible from a generator
    q = make_scene(N, 31, logit=True)
    a, b = {k: v.clone() for k, v in q.items()}, {k: v.clone() for k, v in q.items()}
    inject_noise(a, lr, generator=torch.Generator().manual_seed(4), backend="torch")
    inject_noise(b, lr, generator=torch.Generator().manual_seed(4), backend="torch")
    assert torch.equal(a["means3d"], b["means3d"]) and not torch.equal(a["means3d"], q["means3d"])


def test_every_value_error_and_a_refused_call_changes_nothing():
    N = 300
    p, opt = stepped(make_scene(N, 17))
    before = {k: (v.detach().clone(), opt.state[v]["exp_avg"].clone()) for k, v in p.items()}
    u = draws_for(N, 2)
    calls = {
        "relocate": lambda params=p, o=opt, **kw: relocate_dead(params, o, **{"opacity_space": "linear", "draws": u, "backend": "torch", **kw}),
        "grow": lambda params=p, o=opt, **kw: grow(params, o, **{"cap_max": 10_000, "opacity_space": "linear", "backend": "torch", **kw}),
        "noise": lambda params=p, o=None, **kw: inject_noise(params, 1e-4, **{"opacity_space": "linear", "backend": "torch", **kw}),
    }
    for what, call in calls.items():
        for name in ("means3d", "scales", "quats", "opacities"):
            with pytest.raises(ValueError, match=name):
                call({k: v for k, v in p.items() if k != name}, o=None)
        with pytest.raises(ValueError, match="299 rows"):
            call({**p, "extra": p["extra"].detach()[:299]}, o=None)
        with pytest.raises(ValueError, match="shape"):
            call({**p, "quats": p["means3d"]}, o=None)
        with pytest.raises(ValueError, match="opacities"):
            call({**p, "opacities": torch.rand(N, 2)}, o=None)
        with pytest.raises(ValueError, match="opacity_space"):
            call(opacity_space="sigmoid")
        with pytest.raises(ValueError, match="backend"):
            call(backend="triton")
        with pytest.raises(ValueError, match="dict"):
            call(list(p.values()), o=None)
    for what in ("relocate", "grow"):
        call = calls[what]
        with pytest.raises(ValueError, match="opt's groups"):
            call({k: v for k, v in p.items() if k != "extra"})
        with pytest.raises(ValueError, match="opt's groups"):
            call({**p, "extra": p["extra"].detach().clone()})
        with pytest.raises(ValueError, match="GaussianAdam"):
            call(o=torch.optim.Adam(list(p.values())))
        for bad in (0.0, 1.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="min_opacity"):
                call(min_opacity=bad)
        for bad in (u.float(), u[:5], u.reshape(1, -1), u.to("meta")):
            with pytest.raises(ValueError, match="draws"):
                call(draws=bad)
        with pytest.raises(ValueError, match="sampled"):
            call(draws=None, sampled=torch.zeros(N, dtype=torch.int32))
    with pytest.raises(ValueError, match="cap_max"):
        calls["grow"](cap_max=-1)
    with pytest.raises(ValueError, match="cap_max"):
        calls["grow"](cap_max=1e6)
    with pytest.raises(ValueError, match="growth"):
        calls["grow"](growth=float("inf"))
    noise = torch.randn(N, 3)
    for bad in (noise.double(), noise[:5], noise.reshape(3, N), noise.to("meta")):
        with pytest.raises(ValueError, match="noise"):
            calls["noise"](noise=bad)
    with pytest.raises(ValueError, match="lr"):
        inject_noise(p, float("nan"), opacity_space="linear", backend="torch")
    with pytest.raises(ValueError, match="noise_lr"):
        calls["noise"](noise_lr=float("inf"))
    # backend="hip" (the default) has no fallback: CPU tensors are refused
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        relocate_dead(p, opt, opacity_space="linear", draws=u)
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        grow(p, opt, cap_max=10_000, opacity_space="linear")
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        inject_noise(p, 1e-4, opacity_space="linear", noise=noise)
    for k, v in p.items():
        assert opt.group(k)["params"][0] is v and torch.equal(v.detach(), before[k][0]) and torch.equal(opt.state[v]["exp_avg"], before[k][1])
    assert int(calls["relocate"]().n) > 0                   # and the same call, unbroken, goes through


def test_exports():
    for name in ("relocate_dead", "grow", "inject_noise", "McmcResult"):
        assert name in ms.__all__ and hasattr(ms, name)
    assert ms.relocate_dead is relocate_dead and ms.McmcResult is ms.mcmc.McmcResult


def test_library_exports_and_validates_the_mcmc_entry_points():
    lib = _hip.load()
    for name in ("ms_mcmc_workspace_bytes", "ms_mcmc_sample", "ms_mcmc_apply", "ms_mcmc_noise"):
        assert hasattr(lib, name) and name in _hip.EXPORTS
    assert lib.ms_version() == 5 == _hip.ABI_VERSION
    assert (_hip.MCMC_ROWS, _hip.MCMC_MAX_RATIO, _hip.MCMC_MAX_TENSORS) == (256, 51, 16)
    P, ODD, OFF8 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002), ctypes.c_void_p(0x1004)    # validation never dereferences
    OK, INVALID, WORKSPACE, TOO_LARGE = 0, 1, 2, 3
    err = lambda: lib.ms_last_error_string().decode()
    BIG = 1 << 40
    # cum 8 N, two int64 sums per workgroup, 32 bytes of totals, values 16 N, counts 4 N, flags N, each rounded up to 16
    assert lib.ms_mcmc_workspace_bytes(0) == 0 and lib.ms_mcmc_workspace_bytes(1000) == 8000 + 64 + 32 + 16000 + 4000 + 1008

    def sample(N=1000, opa=P, logit=0, thr=0.005, n_draws=1000, grow_=0, draws=P, sampled_in=None, ws=P, ws_bytes=BIG, s=P, t=P, n=P):
        return lib.ms_mcmc_sample(N, opa, logit, thr, n_draws, grow_, draws, sampled_in, ws, ws_bytes, s, t, n, None)

    assert sample(N=-1) == INVALID and "negative" in err()
    assert sample(n_draws=-1) == INVALID and "negative" in err()
    assert sample(thr=float("nan")) == INVALID and "NaN" in err()
    assert sample(n_draws=999) == INVALID and "relocat" in err()
    for arg in ("opa", "ws", "s", "t"):
        assert sample(**{arg: None}) == INVALID and "null" in err(), arg
    assert sample(draws=None) == INVALID and "null" in err()
    assert sample(opa=ODD) == INVALID and "misaligned" in err()
    assert sample(draws=OFF8) == INVALID and "misaligned" in err()
    assert sample(s=OFF8) == INVALID and "misaligned" in err()
    assert sample(ws=ctypes.c_void_p(0x1008)) == INVALID and "misaligned" in err()
    assert sample(ws_bytes=100) == WORKSPACE and "workspace" in err()
    assert sample(N=0, n_draws=0, opa=None, draws=None, ws=None, s=None, t=None, n=None) == OK
    assert sample(N=1000, n_draws=0, grow_=1, opa=None, draws=None, ws=None, s=None, t=None, n=None) == OK
    assert sample(N=(1 << 31) // 3 + 1, n_draws=(1 << 31) // 3 + 1) == TOO_LARGE and "2^31" in err()

    def apply(N=1000, n_draws=1000, n_rows=1000, grow_=0, ws=P, ws_bytes=BIG, s=P, t=P, n=1, recs=None, values=(None,) * 3,
              min_opacity=0.005, **kw):
        f = dict(base=0x1000, width=3, kind=_hip.MCMC_COPY)
        f.update(kw)
        recs = recs if recs is not None else [_hip.McmcTensor(**f)]
        table = (_hip.McmcTensor * max(len(recs), 1))(*recs)
        return lib.ms_mcmc_apply(N, n_draws, n_rows, grow_, ws, ws_bytes, s, t, n, table, *values, 0, min_opacity, None)

    for field in ("N", "n_draws", "n_rows"):
        assert apply(**{field: -1}) == INVALID and "negative" in err()
    assert apply(n_rows=999) == INVALID and "rows" in err()
    assert apply(n=-1) == INVALID and "n_tensors" in err()
    assert apply(n=17, recs=[_hip.McmcTensor(base=0x1000, width=1, kind=0)] * 17) == INVALID and "n_tensors" in err()
    for arg in ("ws", "s", "t"):
        assert apply(**{arg: None}) == INVALID and "null" in err(), arg
    assert lib.ms_mcmc_apply(1000, 1000, 1000, 0, P, BIG, P, P, 1, None, None, None, None, 0, 0.005, None) == INVALID and "null" in err()
    assert apply(base=None) == INVALID and "null" in err()
    assert apply(base=0x1002) == INVALID and "misaligned" in err()
    assert apply(values=(P, None, P)) == INVALID and "all or none" in err()
    assert apply(n=0) == INVALID and "nothing to do" in err()
    assert apply(values=(P, P, P), min_opacity=0.0) == INVALID and "min_opacity" in err()
    assert apply(values=(P, P, P), min_opacity=float("nan")) == INVALID and "min_opacity" in err()
    assert apply(values=(ODD, P, P)) == INVALID and "misaligned" in err()
    assert apply(s=OFF8) == INVALID and "misaligned" in err()
    assert apply(width=0) == INVALID and "size" in err()
    assert apply(kind=4) == INVALID and "kind" in err()
    assert apply(kind=_hip.MCMC_SCALE, width=4) == INVALID and "width 4" in err()
    assert apply(kind=_hip.MCMC_OPACITY, width=3) == INVALID and "width 3" in err()
    assert apply(ws_bytes=100) == WORKSPACE and "workspace" in err()
    assert apply(N=0, n_draws=0, n_rows=0, ws=None, s=None, t=None, n=0) == OK
    assert apply(n_draws=0, ws=None, s=None, t=None, n=0) == OK
    assert apply(width=1 << 22) == TOO_LARGE and "2^31" in err()
    assert apply(n_rows=1 << 30) == TOO_LARGE and "2^31" in err()

    def noise(N=1000, ptrs=(P,) * 5, step=1.0, k=100.0, x0=0.995):
        return lib.ms_mcmc_noise(N, *ptrs, 0, step, k, x0, None)

    assert noise(N=-1) == INVALID and "negative" in err()
    assert noise(step=float("nan")) == INVALID and "NaN" in err()
    for i in range(5):
        assert noise(ptrs=tuple(None if j == i else P for j in range(5))) == INVALID and "null" in err()
        assert noise(ptrs=tuple(ODD if j == i else P for j in range(5))) == INVALID and "misaligned" in err()
    assert noise(N=0, ptrs=(None,) * 5) == OK
    assert noise(N=1 << 29) == TOO_LARGE and "2^31" in err()
