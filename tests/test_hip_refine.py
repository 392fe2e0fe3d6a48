"""GPU: the fused densification step (csrc/densify.hip; mojosplat_amd/refine.py, densify_and_prune with backend="hip")
against its definition (backend="torch") on the CPU, from the same float32 inputs and the same noise.

``source`` and the four counts are equal; every copied row of every parameter and moment, and the children's scales, are
bit-identical; the children's means are held to the bar of test_hip_optim.py, measured per case against the definition in
float64 and in float32:
    max|hip - def64| <= 4 max|def32 - def64| + 4 eps32 max|def64|
Every parity case prints its (ehip, e32) pair (run with -s); DESIGN.md, section 4d, is where they are recorded."""
import os
import warnings

import pytest
import torch

import mojosplat_amd as ms
from helpers import GOLDEN_DIR, camera_from_golden, load_golden
from mojosplat_amd import DensifyStats, GaussianAdam, _hip, densify_and_prune, photometric_loss
from mojosplat_amd.autograd import render_gaussians_trainable
from mojosplat_amd.refine import child_means_torch
from test_refine_cpu import DEFAULTS, WIDTHS, make_scene

pytestmark = pytest.mark.gpu

EPS32 = torch.finfo(torch.float32).eps
R, SPAN = _hip.DENSIFY_ROWS, _hip.DENSIFY_SCAN_SPAN
KEYS = ("exp_avg", "exp_avg_sq")


def _moments(p, seed=23):
    """{name: (exp_avg, exp_avg_sq)}: what two Adam steps would leave, made up on the CPU so that both sides start from the
    same bits."""
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.randn(v.shape, generator=g) * 1e-3, torch.rand(v.shape, generator=g) * 1e-6) for k, v in p.items()}


def _optimiser(p, moments, backend):
    opt = GaussianAdam(p, lr=1e-3, backend=backend)
    if moments is not None:
        for k, v in p.items():
            opt.state[v] = {"step": torch.tensor(2.0), "exp_avg": moments[k][0].to(v.device).clone(),
                            "exp_avg_sq": moments[k][1].to(v.device).clone()}
    return opt


def _to_device(p, device, misalign=()):
    out = {}
    for k, v in p.items():
        if k in misalign:       # contiguous float32, 4 bytes off a 16-byte boundary: the element path of the move kernel
            out[k] = torch.empty(v.numel() + 1, device=device)[1:].view(v.shape).copy_(v)
            assert out[k].data_ptr() % 16 == 4 and out[k].is_contiguous()
        else:
            out[k] = v.to(device)
        out[k].requires_grad_(True)
    return out


def _both(p, stats, noise, device, opt="stepped", misalign=(), **kw):
    """-> (definition's result on the CPU, its optimiser, HIP result, its optimiser); opt: "stepped", "fresh" or None."""
    moments = _moments(p) if opt == "stepped" else None
    pc = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    oc = _optimiser(pc, moments, "torch") if opt else None
    ref = densify_and_prune(pc, stats, oc, noise=noise, backend="torch", **kw)
    pd = _to_device(p, device, misalign)
    od = _optimiser(pd, moments, "hip") if opt else None
    sd = DensifyStats(0, _buffers=tuple(t.to(device) for t in (stats.grad2d, stats.count, stats.max_radii)))
    torch.cuda.synchronize(device)
    got = densify_and_prune(pd, sd, od, noise=noise.to(device), **kw)      # backend="hip" is the default
    return ref, oc, got, od


def _assert_parity(tag, p, noise, ref, oc, got, od, need_all=True):
    counts = lambda r: (r.n_kept, r.n_cloned, r.n_split, r.n_pruned)
    if need_all:
        assert min(counts(ref)) > 0, f"{tag}: the case does not exercise every kind of row: {counts(ref)}"
    assert counts(got) == counts(ref)
    assert got.source.dtype == torch.int64 and torch.equal(got.source.cpu(), ref.source)
    n_out, first = ref.source.numel(), ref.n_kept + ref.n_cloned
    assert got.stats.n == n_out and got.stats.device == got.source.device
    assert not any(t.any() for t in (got.stats.grad2d, got.stats.count, got.stats.max_radii))
    for k in p:
        h = got.params[k]
        assert h.shape == ref.params[k].shape and h.is_leaf and h.requires_grad and h.is_contiguous()
        if k == "means3d":
            assert torch.equal(h.detach().cpu()[:first], ref.params[k].detach()[:first]), f"{tag} {k}: a copied row differs"
        else:           # (the children's scales included: one float32 subtraction)
            assert torch.equal(h.detach().cpu(), ref.params[k].detach()), f"{tag} {k}: a row differs"
        if od is not None:
            assert od.group(k)["params"][0] is h
            st, want = od.state.get(h), oc.state.get(oc.group(k)["params"][0])
            assert bool(st) == bool(want)
            if st:
                assert int(st["step"]) == int(want["step"])
                for key in KEYS:
                    assert torch.equal(st[key].cpu(), want[key]), f"{tag} {k}.{key} differs"
    if ref.n_split:
        rows = ref.source[first:]
        c = torch.arange(rows.numel()) // ref.n_split
        d64 = child_means_torch(p["means3d"][rows].double(), p["scales"][rows].double(), p["quats"][rows].double(),
                                noise[c, rows].double())
        hip, d32 = got.params["means3d"].detach().cpu()[first:].double(), ref.params["means3d"].detach()[first:].double()
        assert torch.isfinite(hip).all()
        ehip, e32, top = float((hip - d64).abs().max()), float((d32 - d64).abs().max()), float(d64.abs().max())
        print(f"\n[densify {tag}] child means (ehip, e32) = ({ehip:.3g}, {e32:.3g}), max|def64| {top:.3g}; rows {counts(ref)}")
        assert ehip <= 4 * e32 + 4 * EPS32 * top, f"{tag}: ehip {ehip:.3g} > 4 * e32 {e32:.3g} + 4 eps * max|def64| {top:.3g}"


# one N with more workgroups than the scan kernel takes in one pass of its lanes
@pytest.mark.parametrize("N", [0, 1, R - 1, R, R + 1, 3 * R + 17, SPAN * R + 2 * R + 5])
def test_parity_with_the_definition(device, N):
    p, stats, noise = make_scene(N, 100 + N)
    ref, oc, got, od = _both(p, stats, noise, device, **DEFAULTS)
    _assert_parity(f"N{N}", p, noise, ref, oc, got, od, need_all=N > 1)


@pytest.mark.parametrize("case", ["everything pruned", "nothing changes", "every row split"])
def test_degenerate_scenes(device, case):
    N = 2 * R + 9
    p, stats, noise = make_scene(N, 41)
    stats.max_radii.zero_()
    if case == "everything pruned":
        p["opacities"].zero_()
    else:
        p["opacities"].fill_(0.5)
        p["scales"] = p["scales"].clamp(max=-3.0) if case == "every row split" else p["scales"].clamp(max=-5.0)
        p["scales"][:, 0] = -3.0 if case == "every row split" else -5.0
        stats.count.fill_(2.0)
        stats.grad2d.fill_(1e-3 if case == "every row split" else 0.0)
    ref, oc, got, od = _both(p, stats, noise, device, **DEFAULTS)
    want = {"everything pruned": (0, 0, 0, N), "nothing changes": (N, 0, 0, 0), "every row split": (0, 0, N, 0)}[case]
    assert (ref.n_kept, ref.n_cloned, ref.n_split, ref.n_pruned) == want
    _assert_parity(case, p, noise, ref, oc, got, od, need_all=False)
    if case == "nothing changes":
        assert torch.equal(got.source.cpu(), torch.arange(N))
        assert all(torch.equal(got.params[k].detach().cpu(), p[k]) for k in p)
    if case == "everything pruned":
        assert all(got.params[k].shape == (0, *p[k].shape[1:]) for k in p) and got.stats.n == 0
        assert od.state[got.params["scales"]]["exp_avg"].shape == (0, 3)


@pytest.mark.parametrize("opt", ["stepped", "fresh", None])
def test_tensor_table(device, opt):
    """Widths 1, 3, 4, (16, 3) and 5, (N, 1) opacities in logit space, a tensor off 16-byte alignment, and more tensors than
    one table holds (with the moments: 3 x 9 records; without: 20 names)."""
    N = 3 * R + 17
    widths = dict(WIDTHS, opacities=(1,), **{f"t{i}": w for i, w in enumerate([(2,), (8,), (1, 3)])})
    if opt is None:
        widths.update({f"u{i}": (1 + i % 4,) for i in range(11)})
    assert opt == "fresh" or len(widths) * (3 if opt == "stepped" else 1) > _hip.DENSIFY_MAX_TENSORS
    p, stats, noise = make_scene(N, 7, widths=widths, logit=True)
    ref, oc, got, od = _both(p, stats, noise, device, opt=opt, misalign=("features", "quats", "t1"), opacity_space="logit", **DEFAULTS)
    _assert_parity(f"table opt={opt}", p, noise, ref, oc, got, od)
    assert got.params["opacities"].shape == (ref.source.numel(), 1)
    if opt == "fresh":
        assert len(od.state) == 0


def test_two_runs_give_the_same_bits(device):
    N = 40 * R + 3
    p, stats, noise = make_scene(N, 5)
    runs = [_both(p, stats, noise, device, **DEFAULTS)[2:] for _ in range(2)]
    (a, oa), (b, ob) = runs
    assert a.n_split > 0 and torch.equal(a.source, b.source)
    for k in p:
        assert torch.equal(a.params[k], b.params[k])
        for key in KEYS:
            assert torch.equal(oa.state[a.params[k]][key], ob.state[b.params[k]][key])


def test_one_host_wait_and_no_fallback(device):
    p, stats, noise = make_scene(1000, 9)
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        densify_and_prune(p, stats, noise=noise, backend="hip")
    pd = _to_device(p, device)
    sd = DensifyStats(0, _buffers=tuple(t.to(device) for t in (stats.grad2d, stats.count, stats.max_radii)))
    with pytest.raises(ValueError, match="CUDA/ROCm|is on"):
        densify_and_prune(dict(pd, extra=p["extra"]), sd, noise=noise.to(device))
    with pytest.raises(ValueError, match="float32"):
        densify_and_prune(dict(pd, extra=pd["extra"].detach().double()), sd, noise=noise.to(device))
    with pytest.raises(ValueError, match="contiguous"):
        densify_and_prune(dict(pd, extra=torch.randn(5, 1000, device=device).t()), sd, noise=noise.to(device))
    # ONE host wait per call (the totals): in "warn" mode torch reports every synchronising call it sees
    nz = noise.to(device)
    densify_and_prune(pd, sd, noise=nz, **DEFAULTS)                        # (the pinned hand-off buffer exists from here on)
    torch.cuda.synchronize(device)
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            res = densify_and_prune(pd, sd, noise=nz, **DEFAULTS)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    waits = [str(w.message) for w in seen if "synchronizing" in str(w.message)]
    assert len(waits) == 1, waits
    assert res.n_split > 0


def test_training_loop_on_a_golden_scene(device):
    d, c = load_golden(os.path.join(GOLDEN_DIR, "general_cam_n800_250x170.npz"))
    cam = camera_from_golden(d, c, device)
    names = ("means3d", "scales", "quats", "opacities", "features")
    g = torch.Generator().manual_seed(3)
    start = {k: torch.from_numpy(d[k]) for k in names[:4]}
    start["features"] = torch.rand((800, 3), generator=g)
    target = torch.rand((c["H"], c["W"], 3), generator=g).to(device)
    p = {k: v.to(device).clone().requires_grad_(True) for k, v in start.items()}
    opt = GaussianAdam(p, lr={"means3d": 1e-3, "scales": 1e-3, "quats": 1e-3, "opacities": 1e-2, "features": 1e-2})
    stats = DensifyStats(800, device)

    def iteration(p, stats):
        opt.zero_grad()
        img = render_gaussians_trainable(*[p[k] for k in names], cam, densify=stats)
        loss = photometric_loss(img, target)
        loss.backward()
        opt.step()
        return img.detach()

    iteration(p, stats)
    assert float(stats.count.sum()) > 0
    # thresholds from this scene's own statistics, so that every rule fires: the median mean gradient of the Gaussians that
    # were seen, the median largest scale, the 10 % quantile of opacity, the 95 % quantile of the largest scale
    mg, smax = stats.mean_grad().cpu(), p["scales"].detach().cpu().max(-1).values
    rules = dict(grow_grad2d=float(mg[mg > 0].median()), grow_scale3d=float(smax.median().exp()), grow_scale2d=None,
                 prune_opa=float(p["opacities"].detach().cpu().quantile(0.1)), prune_scale3d=float(smax.quantile(0.95).exp()),
                 prune_scale2d=None)
    noise = torch.randn((2, 800, 3), generator=g)
    cpu = densify_and_prune({k: v.detach().cpu() for k, v in p.items()},
                            DensifyStats(0, _buffers=tuple(t.cpu() for t in (stats.grad2d, stats.count, stats.max_radii))),
                            noise=noise, backend="torch", **rules)
    assert min(cpu.n_kept, cpu.n_cloned, cpu.n_split, cpu.n_pruned) >= 1
    res = densify_and_prune(p, stats, opt, noise=noise.to(device), **rules)
    assert (res.n_kept, res.n_cloned, res.n_split, res.n_pruned) == (cpu.n_kept, cpu.n_cloned, cpu.n_split, cpu.n_pruned)
    assert torch.equal(res.source.cpu(), cpu.source)
    n_new = res.n_kept + res.n_cloned + 2 * res.n_split
    assert n_new != 800 and res.stats.n == n_new and all(res.params[k].shape == (n_new, *start[k].shape[1:]) for k in names)
    before = {k: res.params[k].detach().clone() for k in names}
    img = iteration(res.params, res.stats)
    assert img.shape == (c["H"], c["W"], 3) and torch.isfinite(img).all()
    assert float(res.stats.count[res.n_kept:].sum()) > 0                    # new rows were seen by the second view
    for k in names:
        st = opt.state[res.params[k]]
        assert int(st["step"]) == 2 and st["exp_avg"].shape == res.params[k].shape and torch.isfinite(res.params[k]).all()
        assert not torch.equal(res.params[k].detach()[res.n_kept:], before[k][res.n_kept:]), f"{k}: the new rows did not move"
