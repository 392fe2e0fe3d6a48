"""GPU: the MCMC strategy in HIP (csrc/mcmc.hip; mojosplat_amd/mcmc.py with backend="hip") against its definition
(backend="torch") run on the same device, from the same float32 inputs, the same ``draws`` and the same ``noise``.

In linear opacity space ``sampled``, ``targets``, ``n``, every copied row of every parameter and every moment are
bit-identical.  The computed values -- the new opacity o', the new scales, the displacement of ``inject_noise`` -- are
held to the definition evaluated in float64 on the same inputs: the largest relative error of HIP may be at most 4 times
that of the float32 definition (the two evaluate one formula with differently rounded exp, log and pow).  Every such case
prints its (ehip, e32) pair (run with -s); DESIGN.md, section 4e, is where they are recorded."""
import warnings

import pytest
import torch

from mojosplat_amd import GaussianAdam, _hip, grow, inject_noise, photometric_loss, relocate_dead
from mojosplat_amd.autograd import render_gaussians_trainable
from mojosplat_amd.mcmc import dead_and_cum_torch, noise_step_torch
from mojosplat_amd.scenes import randscene_v1
from test_hip_refine import _moments, _optimiser, _to_device
from test_mcmc_cpu import WIDTHS, draws_for, make_scene

pytestmark = pytest.mark.gpu

R = _hip.MCMC_ROWS
KEYS = ("exp_avg", "exp_avg_sq")
VALUES = ("opacities", "scales")


def _pair(p, device, opt="stepped", misalign=()):
    """Two identical copies of the scene on the device, each with its own optimiser: (definition's, HIP's)."""
    moments = _moments(p) if opt == "stepped" else None
    out = []
    for backend in ("torch", "hip"):
        q = _to_device(p, device, misalign)
        out.append((q, _optimiser(q, moments, backend) if opt else None))
    return out


def _rel(x, ref):
    """The largest relative error of x against ref (float64), over the elements whose reference is not 0."""
    ok = ref != 0
    return float(((x.double() - ref)[ok] / ref[ok]).abs().max()) if bool(ok.any()) else 0.0


def _opacity(x, space):
    return torch.sigmoid(x.double()) if space == "logit" else x.double()


def _compare(tag, p0, ref, oref, got, ohip, res_ref, res_hip, space, rows, call64):
    """ref / got: the parameters after the definition's and after HIP's call; rows: the rows whose opacity and scales were
    computed (sources, targets, appended rows); call64: runs the definition in float64 and returns its parameters."""
    for k in ref:
        a, b = ref[k].detach(), got[k].detach()
        assert a.shape == b.shape and b.is_contiguous()
        if k in VALUES:
            keep = torch.ones(a.shape[0], dtype=torch.bool, device=a.device)
            keep[rows] = False
            assert torch.equal(a[keep], b[keep]), f"{tag} {k}: a row nobody drew changed"
        else:
            assert torch.equal(a, b), f"{tag} {k}: a copied row differs"
        if ohip is not None:
            assert ohip.group(k)["params"][0] is got[k]
            st, want = ohip.state.get(got[k]), oref.state.get(ref[k])
            assert bool(st) == bool(want)
            if st:
                assert int(st["step"]) == int(want["step"])
                for key in KEYS:
                    assert torch.equal(st[key], want[key]), f"{tag} {k}.{key} differs"
    if rows.numel():
        d64 = call64()
        for k in VALUES:
            f = (lambda x: _opacity(x, space)) if k == "opacities" else (lambda x: x.double())
            want = f(d64[k].detach().reshape(got[k].shape[0], -1)[rows])
            ehip = _rel(f(got[k].detach().reshape(got[k].shape[0], -1)[rows]), want)
            e32 = _rel(f(ref[k].detach().reshape(ref[k].shape[0], -1)[rows]), want)
            print(f"\n[mcmc {tag}] {k}: (ehip, e32) = ({ehip:.3g}, {e32:.3g}) over {rows.numel()} rows")
            assert torch.isfinite(got[k]).all()
            assert ehip <= 4 * e32, f"{tag} {k}: ehip {ehip:.3g} > 4 * e32 {e32:.3g}"


def _relocate_both(tag, p, device, space="linear", opt="stepped", misalign=(), seed=1, own_draws=True):
    N = p["means3d"].shape[0]
    (ref, oref), (got, ohip) = _pair(p, device, opt, misalign)
    u = draws_for(N, seed).to(device)
    res_hip = relocate_dead(got, ohip, opacity_space=space, draws=u)                   # backend="hip" is the default
    how = dict(draws=u) if own_draws else dict(sampled=res_hip.sampled)
    res_ref = relocate_dead(ref, oref, opacity_space=space, backend="torch", **how)
    n = int(res_hip.n)
    assert res_hip.n.dtype == torch.int64 and res_hip.n.device == u.device and res_hip.params is got
    assert n == int(res_ref.n)
    assert res_hip.sampled.dtype == torch.int64 and torch.equal(res_hip.sampled, res_ref.sampled)
    assert res_hip.targets.dtype == torch.int64 and torch.equal(res_hip.targets, res_ref.targets)
    s = res_hip.sampled[:n]
    rows = torch.unique(torch.cat([s[s >= 0], res_hip.targets[:n][s >= 0]]))

    def call64():
        q = {k: v.double().to(device) for k, v in p.items()}
        relocate_dead(q, opacity_space=space, sampled=res_hip.sampled, backend="torch")
        return q

    _compare(tag, p, ref, oref, got, ohip, res_ref, res_hip, space, rows, call64)
    return res_hip, got


def _scene(N, seed, dead, **kw):
    p = make_scene(N, seed, dead=0.0, **kw)
    g = torch.Generator().manual_seed(seed + 1000)
    lo = 0.001 if not kw.get("logit") else -6.9
    p["opacities"].view(-1)[torch.randperm(N, generator=g)[:dead]] = lo
    return p


# N and the number of dead rows: one workgroup, two, several, and more workgroups than the scan takes in one pass
@pytest.mark.parametrize("N,dead", [(1, 1), (5, 2), (257, 60), (1000, 300), (5000, 2000), (512 * R + 2 * R + 5, 30_000)])
def test_relocate_parity_in_linear_space(device, N, dead):
    p = _scene(N, 100 + N, dead)
    res, got = _relocate_both(f"relocate N{N}", p, device)
    n = int(res.n)
    assert n == (dead if N > 1 else 0)                      # N = 1: the single row is dead, nothing to draw from
    if N == 1:
        assert all(torch.equal(got[k].detach().cpu(), p[k]) for k in p)
    else:
        d = dead_and_cum_torch(p["opacities"], 0.005, "linear")[0]
        assert torch.equal(res.targets[:n].cpu(), torch.nonzero(d).reshape(-1)) and not d[res.sampled[:n].cpu()].any()
        # (a target can sit exactly ON the threshold, where the clamp leaves a source that was drawn often: no more is asked)
        assert float(got["opacities"].detach()[res.targets[:n]].min()) >= float(torch.tensor(0.005, dtype=torch.float32))


def test_one_source_many_targets(device):
    """N = 300 with 200 dead, one live row at opacity 0.99 and the rest at 0.006: that row is drawn more than 51 times."""
    N = 300
    p = make_scene(N, 7, dead=0.0)
    p["opacities"][:] = 0.006
    p["opacities"][torch.randperm(N, generator=torch.Generator().manual_seed(1))[:200]] = 0.001
    star = int(torch.nonzero(p["opacities"] > 0.005)[17])
    p["opacities"][star] = 0.99
    res, got = _relocate_both("one source", p, device)
    assert int(res.n) == 200
    times = int((res.sampled[:200] == star).sum())
    assert times > 51, times
    mine = res.targets[:200][res.sampled[:200] == star]
    for k in p:
        assert torch.equal(got[k].detach()[mine], got[k].detach()[star].expand(times, *p[k].shape[1:]))
    # the ratio is clamped: the same values as 51 draws would give
    from mojosplat_amd.mcmc import relocated_torch
    want, _ = relocated_torch(torch.tensor([0.99], dtype=torch.float64), torch.tensor([51]))
    assert abs(float(got["opacities"].detach()[star]) - float(want)) <= 1e-6 * float(want)


@pytest.mark.parametrize("opt", ["stepped", "fresh", None])
def test_tensor_table(device, opt):
    """Widths 1, 3, 4, (16, 3) and 5, (N, 1) opacities, tensors off 16-byte alignment, and more tensors than one table holds
    (with the moments: 3 x 9 records; without: 20 names)."""
    N = 3 * R + 17
    widths = dict(WIDTHS, opacities=(1,), **{f"t{i}": w for i, w in enumerate([(2,), (8,), (1, 3)])})
    if opt is None:
        widths.update({f"u{i}": (1 + i % 4,) for i in range(11)})
    assert opt == "fresh" or len(widths) * (3 if opt == "stepped" else 1) > _hip.MCMC_MAX_TENSORS
    p = _scene(N, 9, 250, widths=widths)
    res, got = _relocate_both(f"table opt={opt}", p, device, opt=opt, misalign=("features", "quats", "t1", "scales"))
    assert int(res.n) == 250 and got["opacities"].shape == (N, 1)


def test_relocate_in_logit_space(device):
    N = 2000
    p = _scene(N, 13, 700, logit=True)
    res, got = _relocate_both("relocate logit", p, device, space="logit", own_draws=False)
    n = int(res.n)
    d = dead_and_cum_torch(p["opacities"], 0.005, "logit")[0]
    assert n == 700 == int(d.sum())
    s = res.sampled[:n].cpu()
    assert int(s.min()) >= 0 and not d[s].any(), "a dead row was sampled"
    assert torch.equal(res.targets[:n].cpu(), torch.nonzero(d).reshape(-1))
    assert len(set(s.tolist())) > 300                       # (the draws spread over the live rows)


@pytest.mark.parametrize("N,growth,cap,space", [(5, 2.0, 100, "linear"), (1000, 1.05, 10_000, "linear"), (5000, 1.05, 5100, "linear"),
                                                (300, 3.5, 10_000, "linear"), (1000, 1.05, 10_000, "logit")])
def test_grow_parity(device, N, growth, cap, space):
    p = _scene(N, 200 + N, N // 4, logit=space == "logit")
    (ref, oref), (got, ohip) = _pair(p, device)
    n_new = min(cap, int(growth * N)) - N
    u = draws_for(n_new, 3).to(device)
    res_hip = grow(got, ohip, cap_max=cap, growth=growth, opacity_space=space, draws=u)
    how = dict(draws=u) if space == "linear" else dict(sampled=res_hip.sampled)
    res_ref = grow(ref, oref, cap_max=cap, growth=growth, opacity_space=space, backend="torch", **how)
    assert res_hip.n == res_ref.n == n_new > 0
    assert torch.equal(res_hip.sampled, res_ref.sampled) and torch.equal(res_hip.targets, res_ref.targets)
    assert torch.equal(res_hip.targets, torch.arange(N, N + n_new, device=device))
    d = dead_and_cum_torch(p["opacities"], 0.005, space)[0]
    s = res_hip.sampled
    assert int(s.min()) >= 0 and not d[s.cpu()].any()
    for k in p:
        h = res_hip.params[k]
        assert h.shape == (N + n_new, *p[k].shape[1:]) and h.is_leaf and h.requires_grad
        assert torch.equal(h.detach()[N:], h.detach()[s]), f"{k}: the appended rows are not in draw order"
    rows = torch.unique(torch.cat([s, res_hip.targets]))

    def call64():
        q = {k: v.double().to(device) for k, v in p.items()}
        return grow(q, cap_max=cap, growth=growth, opacity_space=space, sampled=res_hip.sampled, backend="torch").params

    _compare(f"grow N{N} {space}", p, res_ref.params, oref, res_hip.params, ohip, res_ref, res_hip, space, rows, call64)
    # the optimiser goes on stepping
    for v in res_hip.params.values():
        v.grad = torch.ones_like(v)
    ohip.step()
    assert int(ohip.state[res_hip.params["means3d"]]["step"]) == 3


def test_grow_with_nothing_alive_and_no_ops(device):
    N = R + 3
    p = make_scene(N, 5, dead=0.0)
    p["opacities"][:] = 0.001
    (ref, oref), (got, ohip) = _pair(p, device)
    u = draws_for(int(1.5 * N) - N, 2).to(device)
    a = grow(got, ohip, cap_max=10_000, growth=1.5, opacity_space="linear", draws=u)
    b = grow(ref, oref, cap_max=10_000, growth=1.5, opacity_space="linear", draws=u, backend="torch")
    assert (a.sampled == -1).all() and torch.equal(a.sampled, b.sampled)
    for k in p:
        assert torch.equal(a.params[k], b.params[k])
        assert torch.equal(a.params[k].detach()[N:].cpu(), p[k][:1].expand(u.numel(), *p[k].shape[1:]))
        for key in KEYS:
            assert torch.equal(ohip.state[a.params[k]][key], oref.state[b.params[k]][key])
    q = _to_device(make_scene(N, 5), device)
    res = grow(q, cap_max=N, opacity_space="linear")
    assert res.n == 0 and res.params is q
    # relocation: nobody dead, and everybody dead
    alive = _to_device(make_scene(N, 6, dead=0.0), device)
    before = {k: v.detach().clone() for k, v in alive.items()}
    res = relocate_dead(alive, opacity_space="linear", draws=draws_for(N, 1).to(device))
    assert int(res.n) == 0 and (res.sampled == -1).all() and (res.targets == -1).all()
    assert all(torch.equal(alive[k].detach(), before[k]) for k in alive)
    before = {k: v.detach().clone() for k, v in got.items()}
    res = relocate_dead(got, opacity_space="linear", draws=draws_for(N, 1).to(device))
    assert int(res.n) == 0 and all(torch.equal(got[k].detach(), before[k]) for k in got)


def test_two_runs_give_the_same_bits(device):
    N = 40 * R + 3
    p = _scene(N, 5, 4000)
    runs = []
    for _ in range(2):
        q = _to_device(p, device)
        opt = _optimiser(q, _moments(p), "hip")
        r = relocate_dead(q, opt, opacity_space="linear", draws=draws_for(N, 4).to(device))
        g = grow(q, opt, cap_max=10 ** 6, opacity_space="linear", draws=draws_for(int(1.05 * N) - N, 5).to(device))
        inject_noise(g.params, 1e-3, opacity_space="linear", noise=torch.randn((g.params["means3d"].shape[0], 3),
                                                                                 generator=torch.Generator().manual_seed(6)).to(device))
        runs.append((r, g, opt))
    (ra, ga, oa), (rb, gb, ob) = runs
    assert int(ra.n) == 4000 and torch.equal(ra.sampled, rb.sampled) and torch.equal(ga.sampled, gb.sampled)
    for k in p:
        assert torch.equal(ga.params[k], gb.params[k])
        for key in KEYS:
            assert torch.equal(oa.state[ga.params[k]][key], ob.state[gb.params[k]][key])


@pytest.mark.parametrize("N,space", [(200, "linear"), (R + 1, "logit"), (5000, "linear"), (5000, "logit")])
def test_inject_noise_parity(device, N, space):
    p = make_scene(N, 300 + N, logit=space == "logit", dead=0.5)       # half the rows nearly transparent: their gate is open
    p["means3d"].zero_()                                                 # the result IS the displacement
    p["scales"] += 2.0 * torch.randn((N, 1), generator=torch.Generator().manual_seed(N))
    noise = torch.randn((N, 3), generator=torch.Generator().manual_seed(N + 1))
    step = 1.6e-4 * 5e5
    misalign = ("quats",) if N == 5000 and space == "logit" else ()                # (the kernel's dword path for the quaternion)
    ref, got = _to_device(p, device, misalign), _to_device(p, device, misalign)
    before = {k: v.detach().clone() for k, v in got.items()}
    version = got["means3d"]._version
    assert inject_noise(got, 1.6e-4, opacity_space=space, noise=noise.to(device)) is None
    inject_noise(ref, 1.6e-4, opacity_space=space, noise=noise.to(device), backend="torch")
    assert got["means3d"]._version > version, "the scene cache would not see the new means"
    assert all(torch.equal(got[k].detach(), before[k]) for k in got if k != "means3d")
    d64 = noise_step_torch(p["scales"].double().to(device), p["quats"].double().to(device), p["opacities"].double().to(device),
                           noise.to(device), step, space)
    top = d64.abs().max(-1, keepdim=True).values
    # a gate below 1e-28 leaves a step that float32 holds as a denormal or as 0 (exp overflows from o = 0.89 on): those rows
    # are only asked to stand still
    moving = top.reshape(-1) > 1e-30
    assert int(moving.sum()) >= (N + 1) // 4
    if not bool(moving.any()):
        assert float(got["means3d"].detach().abs().max()) <= 1e-29
        return
    # relative to the row's largest component: a component that happens to be small next to the others carries their rounding
    ehip = float(((got["means3d"].detach().double() - d64) / top)[moving].abs().max())
    e32 = float(((ref["means3d"].detach().double() - d64) / top)[moving].abs().max())
    print(f"\n[mcmc noise N{N} {space}] displacement: (ehip, e32) = ({ehip:.3g}, {e32:.3g}) over {int(moving.sum())} rows")
    assert torch.isfinite(got["means3d"]).all() and ehip <= 4 * e32, f"ehip {ehip:.3g} > 4 * e32 {e32:.3g}"
    assert float(got["means3d"].detach()[~moving].abs().max() if bool((~moving).any()) else 0.0) <= 1e-29


def test_no_host_wait_and_no_fallback(device):
    N = 1000
    p = _scene(N, 9, 300)
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        relocate_dead(p, opacity_space="linear", backend="hip")
    pd = _to_device(p, device)
    with pytest.raises(ValueError, match="CUDA/ROCm|is on"):
        relocate_dead(dict(pd, extra=p["extra"]), opacity_space="linear")
    with pytest.raises(ValueError, match="float32"):
        grow(dict(pd, extra=pd["extra"].detach().double()), cap_max=5000, opacity_space="linear")
    with pytest.raises(ValueError, match="contiguous"):
        inject_noise(dict(pd, extra=torch.randn(5, N, device=device).t()), 1e-4, opacity_space="linear")
    opt = _optimiser(pd, _moments(p), "hip")
    u, u2 = draws_for(N, 1).to(device), draws_for(50, 2).to(device)
    noise = torch.randn((N, 3), device=device)
    relocate_dead(_to_device(p, device), opacity_space="linear", draws=u)          # (the binomial table is on the device from here on)
    torch.cuda.synchronize(device)
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            inject_noise(pd, 1e-4, opacity_space="linear", noise=noise)
            res = relocate_dead(pd, opt, opacity_space="linear", draws=u)
            grown = grow(pd, opt, cap_max=10_000, opacity_space="linear", draws=u2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    waits = [str(w.message) for w in seen if "synchronizing" in str(w.message)]
    assert waits == [], waits
    assert int(res.n) == 300 and grown.n == 50


def test_training_loop(device):
    """Forty steps of render -> photometric_loss -> GaussianAdam.step -> inject_noise on 400 Gaussians at 64 x 48, with
    relocate_dead and grow every ten steps."""
    N0, W, H, cap = 400, 64, 48, 450
    names = ("means3d", "scales", "quats", "opacities", "features")
    target_scene, cam = randscene_v1(N0, W, H, ell=-1.5, seed=2, device=device)
    with torch.no_grad():
        target = render_gaussians_trainable(*[target_scene[k] for k in names], cam).detach()
    start, _ = randscene_v1(N0, W, H, ell=-1.5, seed=3, device=device)
    start["opacities"][::5] = 1e-4          # a fifth of the rows starts dead, and six steps of 5e-4 leave it below 0.005
    p = {k: start[k].clone().requires_grad_(True) for k in names}
    lrs = {"means3d": 2e-3, "scales": 5e-3, "quats": 1e-3, "opacities": 5e-4, "features": 1e-2}
    opt = GaussianAdam(p, lr=lrs)
    g = torch.Generator(device=device).manual_seed(7)
    losses, relocated = [], 0
    for step in range(40):
        opt.zero_grad()
        loss = photometric_loss(render_gaussians_trainable(*[p[k] for k in names], cam), target)
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
        with torch.no_grad():
            p["opacities"].clamp_(1e-4, 0.999)
        inject_noise(p, lrs["means3d"], noise_lr=5e3, opacity_space="linear", generator=g)
        if step % 10 == 5:
            res = relocate_dead(p, opt, opacity_space="linear", generator=g)
            relocated += int(res.n)
            p = grow(p, opt, cap_max=cap, opacity_space="linear", generator=g).params
            assert p["means3d"].shape[0] <= cap and all(opt.group(k)["params"][0] is p[k] for k in names)
    print(f"\n[mcmc loop] loss {losses[0]:.4f} -> {losses[-1]:.4f}, {relocated} relocated, N {N0} -> {p['means3d'].shape[0]}")
    assert all(torch.isfinite(torch.tensor(losses))) and max(losses[1:]) < losses[0], losses
    assert relocated >= N0 // 5 and p["means3d"].shape[0] == cap
    assert all(torch.isfinite(p[k]).all() for k in names)
    assert all(torch.isfinite(opt.state[p[k]][key]).all() for k in names for key in KEYS)
