"""Several differentiable frames alive at once (multi-view steps): K forwards, then the backwards.

Every other gradient test renders one frame and backpropagates through it at once.  Here K = 3 views of one scene
(tests/live_frames_cases.py) are rendered before any backward runs, the backwards run in any order, and inference frames,
whole training steps, frames whose sorted fronts run out, a release of the cached scratch or another frame's backward sit
in between.  A differentiable frame keeps its own scratch (projected records, lazily sorted lists, per-quad lists, the rows
of raw sums its rasteriser zeroed, its size record) and shares the lane's pinned record, event, buffer hint, pinned clean-up
words, learnt sorting modes and the binning table with every other frame of the thread: whatever leaked from one live
frame into another would leave the images right and the gradients wrong.

Each view is held, on its own, to
  * float64 autograd through the restatement (oracle/torch_oracle.py) on the HIP forward's own visibility and lists, as
    test_hip_backward.py::test_end_to_end_gradients_and_finite_difference builds it: rel=5e-3, ELEM_F64 on every element;
  * the same view rendered and backpropagated ALONE (what every other test does): image bit for bit, gradients within the
    bar of two float32 runs that differ in the order of their atomics (rel=1e-4, FUSED);
and the stacks of faint Gaussians to the per-stage functions with STACKS, as test_hip_backward.py holds them.  Gradients are
compared per view: no per-element comparison lands on a sum over views that nearly cancels.

Largest errors seen on an MI355X (max-norm / worst element): against float64 2.4e-6 / 2.5e-4 (lean), 2.1e-6 / 1.5e-4
(tile_size 8), 2.1e-6 / 3.1e-4 (four channels), 2.1e-6 / 1.6e-4 (per-stage), 1.9e-6 / 2.9e-4 (SH); against the lone frame
8.3e-7 / 4.3e-5 whatever sat between; the stacks against the per-stage functions 2.3e-5 / 2.6e-3, against their lone frames
5.8e-7 / 9.6e-5.  No bar of the suite had to move."""
import gc

import numpy as np
import pytest
import torch

import live_frames_cases as lc
import oracle
from helpers import _posed, assert_grad_close, np_, oracle_project
from oracle import torch_oracle
from test_hip_backward import ELEM_F64, FUSED, STACKS

gpu = pytest.mark.gpu
NAMES = lc.NAMES
K = lc.K

# route -> (what the features are, render_gaussians_trainable's keywords)
ROUTES = {
    "lean": ("rgb", {}),                            # 3 float32 channels, default tile size: lazily sorted fronts, the quad-wave backward
    "ts8": ("rgb", dict(tile_size=8)),              # keeps last_ids, full sorts, the older backward kernel
    "c4": ("c4", {}),                               # 4-channel features
    "stagewise": ("rgb", dict(stagewise=True)),     # _ProjectHip + _RasterizeHip
    "sh": ("sh", dict(sh_degree=3)),                # (N, 16, 3) coefficients through evaluate_sh_hip
}
ORDERS = {"forward": (0, 1, 2), "reversed": (2, 1, 0), "102": (1, 0, 2)}


# ------------------------------------------------------------------ the cases can tell frames apart (no GPU)
def test_the_cameras_can_be_told_apart():
    sc = lc.scene()
    cams = lc.cameras()
    assert len(cams) == K and (cams[0].W, cams[0].H) == (cams[1].W, cams[1].H) == (96, 64) and (cams[2].W, cams[2].H) == (80, 48)
    proj = [oracle_project(oracle, sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], c) for c in cams]
    vis = [(p[3] > 0).all(1) for p in proj]
    for k in range(K):
        assert vis[k].sum() >= lc.MIN_VISIBLE * lc.N, (k, int(vis[k].sum()))
        assert (~vis[k]).sum() >= 8, (k, int((~vis[k]).sum()))      # the zero-gradient assertion of a view has rows to look at
        for j in range(K):
            if j != k:
                assert lc.told_apart(proj[k], proj[j]) >= lc.MIN_APART, (k, j, lc.told_apart(proj[k], proj[j]))
    assert (~vis[0] & ~vis[1] & ~vis[2]).any()                      # ... and so has the one over all views
    # the fourth camera of the pose test looks at the scene too (it WOULD receive a gradient if it were rendered)
    extra = oracle_project(oracle, sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], lc.extra_camera())
    assert (extra[3] > 0).all(1).sum() >= lc.MIN_VISIBLE * lc.N
    assert {len(b) for b in lc.BACKGROUNDS} == {3} and len(set(lc.BACKGROUNDS)) == K


# ------------------------------------------------------------------ inputs, references (computed once, never modified)
def _inputs(device, kind):
    """-> (scene tensors in NAMES order, cameras, cotangents, backgrounds) of a feature kind: rgb | c4 | sh."""
    sc = lc.scene(device, channels=4 if kind == "c4" else 3)
    if kind == "sh":
        sc["features"] = lc.sh_coeffs(device)
    C = 4 if kind == "c4" else 3
    return [sc[n] for n in NAMES], lc.cameras(device), lc.cotangents(device, C), lc.backgrounds(device, C)


def _fresh(tensors):
    return [t.clone().requires_grad_(True) for t in tensors]


def _render(leaves, cam, bg, kw, **more):
    from mojosplat_amd.autograd import render_gaussians_trainable
    return render_gaussians_trainable(*leaves, cam, background_color=bg, **kw, **more)


_F64, _ALONE, _VIS = {}, {}, {}


def _visible(device):
    """(K, N) bool: the HIP projection's own visibility per view."""
    if "v" not in _VIS:
        from mojosplat_amd.autograd import project_gaussians_autograd
        tensors, cams, _, _ = _inputs(device, "rgb")
        with torch.no_grad():
            _VIS["v"] = torch.stack([(project_gaussians_autograd(*tensors[:4], c)[3] > 0).all(1) for c in cams])
    return _VIS["v"]


def _f64(device, kind):
    """Per view: the five float64 gradients of sum(image * cotangent), on the CPU."""
    if kind not in _F64:
        from mojosplat_amd.autograd import project_gaussians_autograd
        from mojosplat_amd.binning import bin_gaussians_to_tiles_hip
        from mojosplat_amd.sh import camera_position
        tensors, cams, vs, bgs = _inputs(device, kind)
        out = []
        for cam, v, bg in zip(cams, vs, bgs):
            with torch.no_grad():
                m2h, conh, deph, radh = project_gaussians_autograd(*tensors[:4], cam)
            ids, ranges = bin_gaussians_to_tiles_hip(m2h, radh, deph, 16, -(-cam.W // 16), -(-cam.H // 16))
            rl = [t.detach().double().cpu().requires_grad_(True) for t in tensors]
            rm2, rcon, _ = torch_oracle.project(rl[0], rl[1], rl[2], cam.view_matrix.double().cpu(), cam.fx, cam.fy, cam.cx,
                                                cam.cy, cam.W, cam.H)
            cols = rl[4] if kind != "sh" else torch_oracle.sh_colors(rl[0], camera_position(cam).double().cpu(), rl[4], 3)
            rimg, _ = torch_oracle.rasterize(rm2, rcon, cols, rl[3], bg.double().cpu(), ranges.cpu(), ids.cpu(), cam.H, cam.W, 16)
            g = torch.autograd.grad((rimg * v.double().cpu()).sum(), rl)
            out.append((rimg.detach(), [t.detach() for t in g]))
        _F64[kind] = out
    return _F64[kind]


def _alone(device, route):
    """Per view: (image, five gradients) of the view rendered and backpropagated at once, nothing in between."""
    if route not in _ALONE:
        kind, kw = ROUTES[route]
        tensors, cams, vs, bgs = _inputs(device, kind)
        out = []
        for cam, v, bg in zip(cams, vs, bgs):
            leaves = _fresh(tensors)
            img = _render(leaves, cam, bg, kw)
            (img * v).sum().backward()
            out.append((img.detach().clone(), [l.grad.clone() for l in leaves]))
        _ALONE[route] = out
    return _ALONE[route]


def _live(device, route, order, between=None):
    """All K frames of a route alive, `between()`, then the backwards in `order` -> (images, {view: five gradients})."""
    kind, kw = ROUTES[route]
    tensors, cams, vs, bgs = _inputs(device, kind)
    leaves = _fresh(tensors)
    imgs = [_render(leaves, cam, bg, kw) for cam, bg in zip(cams, bgs)]
    if between is not None:
        between()
    grads = {}
    for k in order:
        grads[k] = torch.autograd.grad((imgs[k] * vs[k]).sum(), leaves, retain_graph=True)
    return [i.detach() for i in imgs], grads


def _check_views(device, tag, route, imgs, grads):
    """The two bars of every view, and exact zeros where a view (and where every view) culls."""
    kind = ROUTES[route][0]
    f64, alone, vis = _f64(device, kind), _alone(device, route), _visible(device)
    for k in sorted(grads):
        assert torch.equal(imgs[k], alone[k][0]), f"{tag}: view {k}'s image differs from the view rendered alone"
        np.testing.assert_allclose(np_(imgs[k]), np_(f64[k][0]), atol=2e-4)
        for name, g, g64, ga in zip(NAMES, grads[k], f64[k][1], alone[k][1]):
            assert_grad_close(f"{tag}/v{k}/f64/{name}", g, g64, rel=5e-3, elem_rel=ELEM_F64)
            assert_grad_close(f"{tag}/v{k}/alone/{name}", g, ga, rel=1e-4, **FUSED)
            assert g64.abs().max() > 0
            assert (g[~vis[k]] == 0).all(), f"{tag}: view {k} moved a Gaussian it culls ({name})"
    nowhere = ~vis.any(0)
    assert nowhere.any()
    for name, per_view in zip(NAMES, zip(*[grads[k] for k in sorted(grads)])):
        assert all((g[nowhere] == 0).all() for g in per_view), name


def _check_sum(device, tag, route):
    """ONE backward of the summed losses, all frames alive, on fresh leaves: the sum of the float64 per-view gradients
    (max-norm bar only: a sum over views may cancel)."""
    kind, kw = ROUTES[route]
    tensors, cams, vs, bgs = _inputs(device, kind)
    leaves = _fresh(tensors)
    imgs = [_render(leaves, cam, bg, kw) for cam, bg in zip(cams, bgs)]
    sum((img * v).sum() for img, v in zip(imgs, vs)).backward()
    f64 = _f64(device, kind)
    for i, name in enumerate(NAMES):
        assert_grad_close(f"{tag}/sum/{name}", leaves[i].grad, sum(f64[k][1][i] for k in range(K)), rel=5e-3)
    nowhere = ~_visible(device).any(0)
    assert all((l.grad[nowhere] == 0).all() for l in leaves)


# ------------------------------------------------------------------ K views, every route, every order
@gpu
@pytest.mark.parametrize("route,order", [("lean", "forward"), ("lean", "reversed"), ("lean", "102"), ("ts8", "reversed"),
                                         ("c4", "reversed"), ("stagewise", "reversed"), ("sh", "reversed")])
def test_k_views_alive_then_the_backwards(device, route, order):
    tag = f"live/{route}/{order}"
    imgs, grads = _live(device, route, ORDERS[order])
    _check_views(device, tag, route, imgs, grads)
    if order == "reversed":
        _check_sum(device, tag, route)
    if route == "c4":
        # (as test_differentiable_frame_edge_cases holds four channels: to the per-stage functions, at its bar)
        kind, kw = ROUTES[route]
        tensors, cams, vs, bgs = _inputs(device, kind)
        for k in range(K):
            leaves = _fresh(tensors)
            (_render(leaves, cams[k], bgs[k], kw, stagewise=True) * vs[k]).sum().backward()
            for name, g, l in zip(NAMES, grads[k], leaves):
                assert_grad_close(f"{tag}/v{k}/stagewise/{name}", g, l.grad, rel=1e-4, **FUSED)


# ------------------------------------------------------------------ what sits between the forwards and the backwards
_OTHER = {}


def _other_frames(device):
    """The inference scene's images, rendered once before anything of a test is alive: (scene, cameras, [img0, img1])."""
    if "o" not in _OTHER:
        import mojosplat_amd as ms
        sc, _ = lc.other_scene(device)
        cams = lc.other_cameras(device)
        bg = torch.tensor([0.2, 0.1, 0.3], device=device)
        args = [sc[n] for n in NAMES]
        with torch.no_grad():
            ref = [ms.render_gaussians(*args, c, background_color=bg).clone() for c in cams]
        assert not torch.equal(ref[0], ref[1]) and ref[0].abs().sum() > 0
        _OTHER["o"] = (args, cams, bg, ref)
    return _OTHER["o"]


def _inference_between(device):
    import mojosplat_amd as ms
    args, cams, bg, ref = _other_frames(device)

    def between():
        with torch.no_grad():
            a = ms.render_gaussians(*args, cams[0], background_color=bg)
            b = ms.render_gaussians(*args, cams[0], background_color=bg)      # (sync-free on the lane's cached scratch)
            assert torch.equal(a, ref[0]) and torch.equal(b, ref[0])
            pend = ms.render_gaussians(*args, cams[1], background_color=bg, async_op=True)
            assert torch.equal(pend.wait(), ref[1])
            batch = ms.render_gaussians_batch(*args, cams, background_color=bg)
            assert torch.equal(batch[0], ref[0]) and torch.equal(batch[1], ref[1])
    return between


def _training_between(device):
    sc, cam = lc.other_scene(device, train=True)
    bg = torch.tensor([0.05, 0.1, 0.2], device=device)

    def between():
        res = []
        for _ in range(2):
            leaves = _fresh([sc[n] for n in NAMES])
            img = _render(leaves, cam, bg, {})
            img.square().sum().backward()
            res.append((img.detach(), [l.grad for l in leaves]))
        assert torch.equal(res[0][0], res[1][0]) and all(torch.isfinite(g).all() and g.abs().max() > 0 for g in res[1][1])
    return between


def _stack_inputs(device):
    from test_hip_fused import _stack_scene
    sc, _ = _stack_scene(*lc.STACK, device)
    cams = lc.stack_cameras(device)
    bg = torch.tensor([0.2, 0.1, 0.3], device=device)
    vs = [torch.rand(c.H, c.W, 3, generator=torch.Generator().manual_seed(5 + k)).to(device) for k, c in enumerate(cams)]
    return [sc[n] for n in NAMES], cams, vs, bg


_STACK_REF = {}


def _stack_reference(device):
    """Per stack camera: (image, gradients) of the per-stage functions on fully sorted 16-px tiles."""
    if "s" not in _STACK_REF:
        tensors, cams, vs, bg = _stack_inputs(device)
        out = []
        for cam, v in zip(cams, vs):
            leaves = _fresh(tensors)
            img = _render(leaves, cam, bg, dict(stagewise=True))
            img.backward(v)
            out.append((img.detach().clone(), [l.grad.clone() for l in leaves]))
        _STACK_REF["s"] = out
    return _STACK_REF["s"]


def _stack_alone(device):
    """Per stack camera: the gradients of the lean frame rendered and backpropagated at once by a thread that has learnt
    nothing (lazily sorted fronts, the redo launch)."""
    if "a" not in _STACK_REF:
        from mojosplat_amd import _fused
        tensors, cams, vs, bg = _stack_inputs(device)
        out = []
        for cam, v in zip(cams, vs):
            _fused._state.clear()
            leaves = _fresh(tensors)
            _render(leaves, cam, bg, {}).backward(v)
            out.append([l.grad.clone() for l in leaves])
        _STACK_REF["a"] = out
    return _STACK_REF["a"]


def _check_stack(tag, k, img, grads, ref, alone=None):
    assert torch.equal(img, ref[k][0]), f"{tag}: stack view {k}"
    for i, (name, g, gr) in enumerate(zip(NAMES, grads, ref[k][1])):
        assert_grad_close(f"{tag}/stack{k}/{name}", g, gr, rel=2e-3, **STACKS)
        if alone is not None:
            assert_grad_close(f"{tag}/stack{k}/alone/{name}", g, alone[k][i], rel=1e-4, **FUSED)


def _redone_bins(device):
    """What the last lazily sorted differentiable frame's backward left in the thread's pinned clean-up words."""
    from mojosplat_amd import _fused
    st = _fused._dev_state(device, 0)
    torch.cuda.synchronize(device)
    w = st.get("own_redo_np")
    return 0 if w is None else int(w[0]) - int(w[1])


@gpu
@pytest.mark.parametrize("what", ["inference", "training", "stranded"])
def test_other_frames_between_the_forwards_and_the_backwards(device, what):
    from mojosplat_amd import _fused
    ref, salone = (_stack_reference(device), _stack_alone(device)) if what == "stranded" else (None, None)
    _alone(device, "lean"), _f64(device, "rgb"), _other_frames(device)
    _fused._state.clear()     # (a thread that has learnt nothing: the stack frame below takes lazily sorted fronts)
    if what == "inference":
        between = _inference_between(device)
    elif what == "training":
        between = _training_between(device)
    else:
        tensors, cams, vs, bg = _stack_inputs(device)

        def between():
            leaves = _fresh(tensors)
            img = _render(leaves, cams[0], bg, {})
            img.backward(vs[0])
            _check_stack("between", 0, img.detach(), [l.grad for l in leaves], ref, salone)
            assert _redone_bins(device) > 0, "the stack frame's backward ran no redo launch: nothing wrote the pinned words"
    imgs, grads = _live(device, "lean", ORDERS["102"], between)
    _check_views(device, f"live/between-{what}", "lean", imgs, grads)


@gpu
def test_two_frames_with_stranded_fronts_alive_together(device):
    """Both backwards run the redo launch, which sorts the frame's keys in place and writes the thread's ONE pair of pinned
    clean-up words; views of the regular scene are alive around them."""
    from mojosplat_amd import _fused
    ref, salone = _stack_reference(device), _stack_alone(device)
    # (the two views are no near copies of each other: nobody passes on the other frame's lists)
    assert all(not torch.allclose(a, b, rtol=0.1, atol=0.0) for a, b in zip(*salone))
    tensors, cams, vs, bg = _stack_inputs(device)
    _alone(device, "lean"), _f64(device, "rgb")
    _fused._state.clear()
    res = {}

    def between():
        leaves = _fresh(tensors)
        simgs = [_render(leaves, cam, bg, {}) for cam in cams]
        for k in (1, 0):
            res[k] = (simgs[k].detach(), torch.autograd.grad(simgs[k], leaves, vs[k], retain_graph=True))
            assert _redone_bins(device) > 0, k
    imgs, grads = _live(device, "lean", ORDERS["reversed"], between)
    for k in (0, 1):
        _check_stack("together", k, *res[k], ref, salone)
    _check_views(device, "live/stranded-together", "lean", imgs, grads)


@gpu
@pytest.mark.parametrize("how", ["release_scratch", "state_clear"])
def test_scratch_released_between_the_forwards_and_the_backwards(device, how):
    """A differentiable frame owns its scratch: giving the thread's cached scratch back leaves it intact."""
    import mojosplat_amd as ms
    from mojosplat_amd import _fused
    args, cams, bg, ref = _other_frames(device)
    with torch.no_grad():
        ms.render_gaussians(*args, cams[0], background_color=bg)     # (the lane HAS cached scratch to give back)

    def between():
        if how == "release_scratch":
            ms.release_scratch()
        else:
            _fused._state.clear()
        # (whatever the allocator hands out next may be the released blocks: fill them)
        junk = torch.full((8 << 20,), float("nan"), device=device)
        del junk
    imgs, grads = _live(device, "lean", ORDERS["reversed"], between)
    _check_views(device, f"live/{how}", "lean", imgs, grads)
    with torch.no_grad():
        assert torch.equal(ms.render_gaussians(*args, cams[0], background_color=bg), ref[0])


@gpu
def test_a_second_backward_after_other_work(device):
    """retain_graph=True on view 0, a whole forward and backward of view 1, then view 0's backward again."""
    tensors, cams, vs, bgs = _inputs(device, "rgb")
    alone = _alone(device, "lean")
    leaves = _fresh(tensors)
    img0 = _render(leaves, cams[0], bgs[0], {})
    first = torch.autograd.grad((img0 * vs[0]).sum(), leaves, retain_graph=True)
    l1 = _fresh(tensors)
    img1 = _render(l1, cams[1], bgs[1], {})
    (img1 * vs[1]).sum().backward()
    second = torch.autograd.grad((img0 * vs[0]).sum(), leaves)
    assert torch.equal(img0.detach(), alone[0][0]) and torch.equal(img1.detach(), alone[1][0])
    for name, a, b, ga, g1, ga1 in zip(NAMES, first, second, alone[0][1], l1, alone[1][1]):
        assert_grad_close(f"live/second/{name}", b, a, rel=1e-4, **FUSED)
        assert_grad_close(f"live/second/alone/{name}", b, ga, rel=1e-4, **FUSED)
        assert_grad_close(f"live/second/view1/{name}", g1.grad, ga1, rel=1e-4, **FUSED)


# ------------------------------------------------------------------ shared statistics, own poses
@gpu
@pytest.mark.parametrize("route", ["lean", "stagewise"])
def test_shared_statistics_and_own_poses(device, route):
    from mojosplat_amd.densify import DensifyStats
    kind, kw = ROUTES[route]
    tensors, cams, vs, bgs = _inputs(device, kind)
    alone = []
    for k in range(K):
        leaves, st, pcam = _fresh(tensors), DensifyStats(lc.N, device), _posed(cams[k])
        (_render(leaves, pcam, bgs[k], kw, densify=st) * vs[k]).sum().backward()
        alone.append(([l.grad for l in leaves], st, pcam.view_matrix.grad.clone()))
    leaves, stats = _fresh(tensors), DensifyStats(lc.N, device)
    pcams = [_posed(c) for c in cams]
    idle = _posed(lc.extra_camera(device))
    imgs = [_render(leaves, pc, bg, kw, densify=stats) for pc, bg in zip(pcams, bgs)]
    for k in ORDERS["102"]:
        (imgs[k] * vs[k]).sum().backward()
    assert torch.equal(stats.count, sum(a[1].count for a in alone))
    assert stats.count.max() == K and (stats.count == 0).any()
    assert torch.equal(stats.max_radii, torch.stack([a[1].max_radii for a in alone]).max(0).values)
    assert_grad_close(f"live/{route}/grad2d", stats.grad2d, sum(a[1].grad2d for a in alone), rel=1e-4, **FUSED)
    for k in range(K):
        g = pcams[k].view_matrix.grad
        assert g is not None and g.abs().max() > 0
        assert_grad_close(f"live/{route}/viewmat{k}", g, alone[k][2], rel=1e-4, **FUSED)
        for j in range(K):     # (the cases' poses differ: nobody can pass with another camera's gradient)
            assert j == k or not torch.allclose(g, alone[j][2], rtol=1e-2, atol=0.0)
    assert idle.view_matrix.grad is None
    for i, name in enumerate(NAMES):
        assert_grad_close(f"live/{route}/posed-sum/{name}", leaves[i].grad, sum(a[0][i] for a in alone), rel=1e-4)


# ------------------------------------------------------------------ losses alive together
@gpu
def test_losses_alive_together(device):
    """K photometric losses (each keeps its workspace for its backward) on K live frames, one backward on their mean."""
    from mojosplat_amd import photometric_loss
    tensors, cams, _, bgs = _inputs(device, "rgb")
    targets = lc.targets(device)
    res = []
    for backend in ("hip", "torch"):
        leaves = _fresh(tensors)
        imgs = [_render(leaves, cam, bg, {}) for cam, bg in zip(cams, bgs)]
        losses = [photometric_loss(img, t, backend=backend) for img, t in zip(imgs, targets)]
        (sum(losses) / K).backward()
        res.append(([float(l.detach()) for l in losses], [l.grad for l in leaves]))
    for a, b in zip(*[r[0] for r in res]):
        assert abs(a - b) <= 1e-5 * abs(b), (a, b)
    assert len({round(v, 6) for v in res[1][0]}) == K
    for name, a, b in zip(NAMES, res[0][1], res[1][1]):
        assert b.abs().max() > 0
        assert_grad_close(f"live-loss/{name}", a, b)


# ------------------------------------------------------------------ nothing outlives the step
@gpu
def test_nothing_outlives_the_step(device):
    from mojosplat_amd import _hip
    tensors, cams, vs, bgs = _inputs(device, "rgb")
    L = _hip.lib()
    # (a frame's workspace on the coarsest grid a lean frame may be binned on: the smallest any of the views can own)
    ws_min = min(L.ms_render_workspace_bytes(lc.N, -(-c.W // 64), -(-c.H // 64)) for c in cams)
    assert ws_min > 4 * max(c.W * c.H for c in cams) * 4 * 4     # ... and it dwarfs what a frame keeps beside it

    def settle():
        gc.collect()
        torch.cuda.synchronize(device)
        return torch.cuda.memory_allocated(device)

    def step():
        leaves = _fresh(tensors)
        before = torch.cuda.memory_allocated(device)
        imgs = [_render(leaves, cam, bg, {}) for cam, bg in zip(cams, bgs)]
        alive = torch.cuda.memory_allocated(device) - before
        sum((img * v).sum() for img, v in zip(imgs, vs)).backward()
        assert alive >= K * ws_min, f"{K} live frames hold {alive} B: less than {K} workspaces of {ws_min} B"
        assert all(l.grad.abs().max() > 0 for l in leaves)
    step()
    base = settle()
    for rep in range(3):
        step()
        assert settle() == base, rep
