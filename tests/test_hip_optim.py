"""GPU: the fused Adam step (csrc/adam.hip; mojosplat_amd/optim.py, GaussianAdam with backend="hip") against its definition.

Every x of (parameter, exp_avg, exp_avg_sq) of every tensor is held to the definition (backend="torch") evaluated in
float64 on the CPU from the same float32 inputs, with a bar MEASURED per case against the same definition in float32:
    max|x_hip - x64| <= 4 max|x32 - x64| + 4 eps32 max|x64|
(the factor 4: a different rounding order of the same float32 operations).  Gradient elements are exactly 0 or of
magnitude in [1e-8, 1e2], so that g*g stays a normal float32 and nothing hinges on denormal handling.  Masks: masked rows
bit-identical to before, visible rows bit-identical to the dense HIP step.  Every case prints its largest (ehip, e32) pair
per quantity (run with -s); DESIGN.md, section 4c, is where they are recorded."""
import math
import os

import pytest
import torch

import mojosplat_amd as ms
from helpers import GOLDEN_DIR, camera_from_golden, load_golden
from mojosplat_amd import GaussianAdam, photometric_loss
from mojosplat_amd.autograd import render_gaussians_trainable

pytestmark = pytest.mark.gpu

EPS32 = torch.finfo(torch.float32).eps
LRS = {"means3d": 1.6e-4, "scales": 5e-3, "quats": 1e-3, "opacities": 5e-2, "features": 2.5e-3, "rgb": 1e-2, "dc": 2.5e-3}
KEYS = ("param", "exp_avg", "exp_avg_sq")


def _shapes(N):
    return {"means3d": (N, 3), "scales": (N, 3), "quats": (N, 4), "opacities": (N,), "features": (N, 16, 3), "rgb": (N, 3),
            "dc": (N, 1, 3)}


def _gradient(shape, gen):
    """float32: every element exactly 0 (one in ten; and every element of one row in five) or of magnitude 10^U(-8, 2)."""
    mag = 10.0 ** (torch.rand(shape, generator=gen, dtype=torch.float64) * 10.0 - 8.0)
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)
    g = (mag * sign).float().clamp(-1e2, 1e2)
    g = torch.where(g.abs() < 1e-8, torch.full_like(g, 1e-8) * sign.float(), g)
    g[torch.rand(shape, generator=gen) < 0.1] = 0
    g[torch.rand(shape[0], generator=gen) < 0.2] = 0
    assert ((g == 0) | ((g.abs() >= 1e-8) & (g.abs() <= 1e2))).all()
    return g


def _inputs(shapes, steps, seed):
    gen = torch.Generator().manual_seed(seed)
    params = {k: torch.randn(s, generator=gen) for k, s in shapes.items()}
    grads = [{k: _gradient(s, gen) for k, s in shapes.items()} for _ in range(steps)]
    return params, grads


def _lrs(shapes):
    return {k: LRS.get(k, 3e-3) for k in shapes}


def _drive(params, grads, backend, dtype, device, masks=None, skip=()):
    """Run len(grads) steps from `params` (float32, CPU) -> {name: (param, exp_avg, exp_avg_sq)} on the CPU, + the optimiser."""
    p = {k: v.to(device=device, dtype=dtype).clone().requires_grad_(True) for k, v in params.items()}
    opt = GaussianAdam(p, lr=_lrs(p), betas=(0.9, 0.999), eps=1e-15, backend=backend)
    for i, g in enumerate(grads):
        for k in p:
            p[k].grad = None if k in skip else g[k].to(device=device, dtype=dtype)
        m = None if masks is None or masks[i] is None else masks[i].to(device)
        opt.step(visibility=m)
    out = {}
    for k in p:
        st = opt.state.get(p[k])
        out[k] = (p[k].detach().cpu(),) + ((st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()) if st else (None, None))
    return out, opt, p


def _assert_bar(tag, hip, x32, x64):
    worst = {}
    for k in x64:
        for i, key in enumerate(KEYS):
            if x64[k][i] is None:
                assert hip[k][i] is None and x32[k][i] is None
                continue
            h, a, b = hip[k][i].double(), x32[k][i].double(), x64[k][i]
            assert h.shape == b.shape and torch.isfinite(h).all()
            ehip, e32, ref = float((h - b).abs().max()), float((a - b).abs().max()), float(b.abs().max())
            if key not in worst or ehip > worst[key][0]:
                worst[key] = (ehip, e32, ref, k)
            assert ehip <= 4 * e32 + 4 * EPS32 * ref, \
                f"{tag} {k}.{key}: ehip {ehip:.3g} > 4 * e32 {e32:.3g} + 4 eps * max|x64| {ref:.3g}"
    print(f"\n[adam {tag}] largest (ehip, e32) pairs: " +
          "; ".join(f"{key} ({w[0]:.3g}, {w[1]:.3g}) max|x64| {w[2]:.3g} on {w[3]}" for key, w in worst.items()))


def _check_case(tag, shapes, steps, seed, device, skip=()):
    params, grads = _inputs(shapes, steps, seed)
    x64, _, _ = _drive(params, grads, "torch", torch.float64, "cpu", skip=skip)
    x32, _, _ = _drive(params, grads, "torch", torch.float32, "cpu", skip=skip)
    hip, opt, p = _drive(params, grads, "hip", torch.float32, device, skip=skip)
    _assert_bar(tag, hip, x32, x64)
    return hip, opt, p, params


@pytest.mark.parametrize("steps", [1, 20])
@pytest.mark.parametrize("N", [1, 7, 1000, 100003])
def test_values_against_the_float64_definition(device, N, steps):
    _, opt, p, _ = _check_case(f"N{N} steps{steps}", _shapes(N), steps, 10 * N + steps, device)
    for k in p:
        assert int(opt.state[p[k]]["step"]) == steps and opt.state[p[k]]["step"].device.type == "cpu"


def test_nine_tensors_take_two_chunks_and_a_missing_gradient_is_skipped(device):
    N = 1000
    shapes = {f"t{i}": s for i, s in enumerate([(N, 3), (N,), (N, 4), (N, 16, 3), (N, 3), (N, 1, 3), (N, 2), (N, 5), (N, 48), (N, 7)])}
    hip, opt, p, params = _check_case("9 of 10 tensors", shapes, 3, 77, device, skip=("t4",))
    assert sum(1 for k in p if p[k] in opt.state) == 9
    assert p["t4"] not in opt.state and torch.equal(hip["t4"][0], params["t4"])
    assert all(int(opt.state[p[k]]["step"]) == 3 for k in p if k != "t4")


def _state_before_the_step(N, device, misalign=False):
    """A GaussianAdam after two dense steps (non-trivial moments) with the third step's gradients attached."""
    shapes = _shapes(N)
    params, grads = _inputs(shapes, 3, 5)
    if misalign:     # contiguous float32, but 4 bytes off a 16-byte boundary: the element-by-element form of the kernel
        p = {k: torch.empty(v.numel() + 1, device=device)[1:].view(v.shape).copy_(v).requires_grad_(True) for k, v in params.items()}
        assert all(t.data_ptr() % 16 == 4 and t.is_contiguous() for t in p.values())
    else:
        p = {k: v.to(device).clone().requires_grad_(True) for k, v in params.items()}
    opt = GaussianAdam(p, lr=_lrs(p), backend="hip")
    for g in grads:
        for k in p:
            p[k].grad = g[k].to(device)
        if g is not grads[-1]:
            opt.step()
    return p, opt


def _snapshot(p, opt):
    return {k: (p[k].detach().clone(), opt.state[p[k]]["exp_avg"].clone(), opt.state[p[k]]["exp_avg_sq"].clone()) for k in p}


def _masks(N, device):
    gen = torch.Generator().manual_seed(N)
    r = torch.rand(N, generator=gen)
    block = torch.zeros(N, dtype=torch.bool)
    block[N // 3: N // 3 + max(1, N // 4)] = True
    out = {"0%": torch.zeros(N, dtype=torch.bool), "10%": r < 0.1, "50%": r < 0.5, "100%": torch.ones(N, dtype=torch.bool),
           "block": block, "50% uint8": (r < 0.5).to(torch.uint8) * 255}
    return {k: v.to(device) for k, v in out.items()}


@pytest.mark.parametrize("N", [7, 1000, 100003])
def test_masks_leave_masked_rows_alone_and_give_visible_rows_the_dense_bits(device, N):
    p, opt = _state_before_the_step(N, device)
    before = _snapshot(p, opt)
    opt.step()
    dense = _snapshot(p, opt)
    p2, opt2 = _state_before_the_step(N, device)
    assert all(torch.equal(a, b) for k in p for a, b in zip(_snapshot(p2, opt2)[k], before[k]))   # the same state, bit for bit
    opt2.step()
    again = _snapshot(p2, opt2)
    assert all(torch.equal(a, b) for k in p for a, b in zip(again[k], dense[k])), "two runs from the same state differ"
    pm_, om_ = _state_before_the_step(N, device, misalign=True)
    om_.step()
    off = _snapshot(pm_, om_)
    assert all(torch.equal(a, b) for k in p for a, b in zip(off[k], dense[k])), "misaligned tensors give other bits"
    for name, mask in _masks(N, device).items():
        pm, om = _state_before_the_step(N, device)
        om.step(visibility=mask)
        got = _snapshot(pm, om)
        vis = mask != 0
        for k in p:
            for i, key in enumerate(KEYS):
                assert torch.equal(got[k][i][~vis], before[k][i][~vis]), f"mask {name}: a masked row of {k}.{key} changed"
                assert torch.equal(got[k][i][vis], dense[k][i][vis]), f"mask {name}: a visible row of {k}.{key} is not the dense step's"
                if name == "100%":
                    assert torch.equal(got[k][i], dense[k][i])
            assert int(om.state[pm[k]]["step"]) == 3
    with pytest.raises(ValueError, match="visibility mask of"):
        opt.step(visibility=torch.ones(N + 1, dtype=torch.bool, device=device))
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        opt.step(visibility=torch.ones(N, dtype=torch.bool))
    assert all(torch.equal(a, b) for k in p for a, b in zip(_snapshot(p, opt)[k], dense[k]))     # a refused step changes nothing
    assert int(opt.state[p["rgb"]]["step"]) == 3


def test_hip_backend_refuses_what_it_cannot_do(device):
    x = torch.randn(10, 3, device=device)
    with pytest.raises(ValueError, match="float32"):
        GaussianAdam({"a": x.double().requires_grad_(True)}, backend="hip")
    with pytest.raises(ValueError, match="float32"):
        GaussianAdam({"a": x.half().requires_grad_(True)}, backend="hip")
    with pytest.raises(ValueError, match="contiguous"):
        GaussianAdam({"a": torch.randn(3, 10, device=device).t().requires_grad_(True)}, backend="hip")
    with pytest.raises(ValueError, match="CUDA/ROCm"):
        GaussianAdam({"a": x.clone().requires_grad_(True), "b": torch.randn(10, requires_grad=True)}, backend="hip")


def test_step_on_another_stream_with_a_dependent_read(device):
    N = 100003
    params, grads = _inputs(_shapes(N), 1, 31)
    ref, _, _ = _drive(params, grads, "hip", torch.float32, device)
    p = {k: v.to(device).clone().requires_grad_(True) for k, v in params.items()}
    opt = GaussianAdam(p, lr=_lrs(p), backend="hip")
    for k in p:
        p[k].grad = grads[0][k].to(device)
    torch.cuda.synchronize(device)
    side = torch.cuda.Stream(device)
    torch.cuda.set_sync_debug_mode("error")          # no host wait inside step
    try:
        with torch.cuda.stream(side):
            opt.step()
            sums = {k: p[k].detach().double().sum() for k in p}      # a dependent read on the same stream
            copies = {k: p[k].detach().clone() for k in p}
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side.synchronize()
    for k in p:
        assert torch.equal(copies[k].cpu(), ref[k][0])
        assert float(sums[k]) == float(ref[k][0].to(device).double().sum())


# ---------------------------------------------------------------------------------------------------- end to end
NAMES = ("means3d", "scales", "quats", "opacities", "features")
E2E_LR = {"means3d": 1e-3, "scales": 1e-4, "quats": 1e-4, "opacities": 1e-4, "features": 1e-2}


def _golden_scene(device):
    d, c = load_golden(os.path.join(GOLDEN_DIR, "randscene_n5000_640x360.npz"))
    cam = camera_from_golden(d, c, device)
    sc = {k: torch.from_numpy(d[k]).to(device) for k in ("means3d", "scales", "quats", "opacities")}
    sc["features"] = torch.from_numpy(d["colors"]).to(device)
    return sc, cam


def _perturbed(sc, seed=11):
    g = torch.Generator().manual_seed(seed)
    out = dict(sc)
    out["means3d"] = sc["means3d"] + 0.02 * torch.randn(sc["means3d"].shape, generator=g).to(sc["means3d"].device)
    out["features"] = (sc["features"] + 0.1 * torch.randn(sc["features"].shape, generator=g).to(sc["features"].device)).clamp(0, 1)
    return out


def _iteration(p, opt, cam, target, bg, masked):
    opt.zero_grad()
    img = render_gaussians_trainable(*[p[k] for k in NAMES], cam, background_color=bg)
    loss = photometric_loss(img, target)
    loss.backward()
    vis = None
    if masked:
        radii = ms.project_gaussians(p["means3d"].detach(), p["scales"].detach(), p["quats"].detach(), p["opacities"].detach(),
                                     cam, backend="hip")[3]
        vis = (radii > 0).all(-1) if radii.dim() == 2 else radii > 0
    grads = {k: p[k].grad.detach().cpu().clone() for k in NAMES}
    opt.step(visibility=vis)
    return float(loss.detach()), grads, vis


def _replay(start, grads, dtype, relocation=None, after=None):
    """The definition on the CPU, driven by recorded gradients (and, optionally, one relocate followed by more steps)."""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in start.items()}
    opt = GaussianAdam(p, lr=E2E_LR, backend="torch")
    for g in grads:
        for k in p:
            p[k].grad = g[k].to(dtype)
        opt.step()
    if relocation is not None:
        keep, fresh = relocation
        p = {k: torch.cat([p[k].detach()[keep], fresh[k].to(dtype)]).requires_grad_(True) for k in p}
        opt.relocate(p, keep, fresh["means3d"].shape[0])
        for g in after:
            for k in p:
                p[k].grad = g[k].to(dtype)
            opt.step()
    return {k: (p[k].detach(), opt.state[p[k]]["exp_avg"], opt.state[p[k]]["exp_avg_sq"]) for k in p}


def test_end_to_end_training_dense_masked_and_after_a_relocate(device):
    sc, cam = _golden_scene(device)
    bg = torch.zeros(3, device=device)
    with torch.no_grad():
        target = ms.render_gaussians(*[sc[k] for k in NAMES], cam, background_color=bg, backend="hip")
    start = {k: _perturbed(sc)[k].cpu() for k in NAMES}
    results = {}
    for masked in (False, True):
        p = {k: start[k].to(device).clone().requires_grad_(True) for k in NAMES}
        opt = GaussianAdam(p, lr=E2E_LR, backend="hip")
        losses, recorded, shares = [], [], []
        for _ in range(30):
            loss, grads, vis = _iteration(p, opt, cam, target, bg, masked)
            losses.append(loss)
            recorded.append(grads)
            if vis is not None:
                shares.append(float(vis.float().mean()))
        with torch.no_grad():
            final = float(photometric_loss(render_gaussians_trainable(*[p[k] for k in NAMES], cam, background_color=bg), target))
        print(f"\n[adam e2e {'masked' if masked else 'dense'}] loss {losses[0]:.5f} -> {final:.5f}" +
              (f", visible share {min(shares):.3f}..{max(shares):.3f}" if shares else ""))
        assert math.isfinite(final) and final < losses[0]
        results[masked] = (p, opt, recorded)
    # the dense run against the definition driven by the same gradients
    p, opt, recorded = results[False]
    hip = {k: (p[k].detach().cpu(), opt.state[p[k]]["exp_avg"].cpu(), opt.state[p[k]]["exp_avg_sq"].cpu()) for k in NAMES}
    _assert_bar("e2e 30 steps", hip, _replay(start, recorded, torch.float32), _replay(start, recorded, torch.float64))
    # densify: drop every tenth row, append 50 (split copies of the first 50, nudged), one more iteration
    N = p["means3d"].shape[0]
    keep = torch.arange(N)[torch.arange(N) % 10 != 3]
    fresh = {k: start[k][:50].clone() for k in NAMES}
    fresh["means3d"] = fresh["means3d"] + 0.01
    newp = {k: torch.cat([p[k].detach()[keep.to(device)], fresh[k].to(device)]).requires_grad_(True) for k in NAMES}
    opt.relocate(newp, keep.to(device), 50)
    assert newp["means3d"].shape[0] == N - N // 10 + 50 == opt.state[newp["features"]]["exp_avg"].shape[0]
    loss, grads, _ = _iteration(newp, opt, cam, target, bg, False)
    assert math.isfinite(loss) and int(opt.state[newp["means3d"]]["step"]) == 31
    hip = {k: (newp[k].detach().cpu(), opt.state[newp[k]]["exp_avg"].cpu(), opt.state[newp[k]]["exp_avg_sq"].cpu()) for k in NAMES}
    _assert_bar("e2e relocate + 1 step", hip, _replay(start, recorded, torch.float32, (keep, fresh), [grads]),
                _replay(start, recorded, torch.float64, (keep, fresh), [grads]))
