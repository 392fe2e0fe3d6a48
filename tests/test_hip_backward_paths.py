"""GPU: every path of the backward rasteriser (and the projection backward's C-ABI options) against float64 autograd of
oracle/torch_oracle.py.

The backward is a dispatch, not one kernel (csrc/rasterize_bwd.hip ms::rasterize_bwd, csrc/pipeline.hip ms_render_bwd,
mojosplat_amd/autograd.py `lean`):

  k_rasterize_bwd_quads (rasterize_bwdq.hip)      fused frame, C = 3, fp32, tile size % 16 == 0 (test_hip_backward.py)
  k_rasterize_bwd_v2<3,4,false>                   packed rows, C <= 3, per-stage / ABI with a workspace / fused C = 1, 2
  k_rasterize_bwd_v2<3,4,true>                    packed rows staged from the frame's records: fused C = 3 at ts 8 / 24
  k_rasterize_bwd_v2<4,4,false>                   packed rows, C = 4
  k_rasterize_bwd<3|4|8|16|32>                    one atomic per component: C >= 5, or no / a too small workspace
  k_unpack_grads<true|false>                      packed rows -> the caller's tensors, overwrite = 1 | 0
  ms_render_bwd non-packed branch                 fused frame, C > 4: memset, v1, ms_project_gaussians_bwd with radii
  k_project_ewa_bwd<0>                            ms_project_gaussians_bwd: linear scales, v_depths = NULL

Comparisons on the GPU's own forward lists: the C oracle projects and bins (or the HIP forward does, for the fused frame),
the same fp32 means2d / conics go to the kernel and, promoted to float64, to torch_oracle.rasterize, and the same upstream
gradient is back-propagated through both.

Branch guard.  A pixel where one of the compositor's branches (alpha >= 1/255, T(1 - alpha) <= 1e-4, sigma < 0; the oracle's
`margin`) or the 0.999 clamp (no geometry gradient beyond it) sits within 1e-5 of its threshold may take the other side in
fp32 than in float64.  Every gradient term a pixel contributes is proportional to its upstream value, so such pixels get a
zero upstream gradient: a flipped branch there moves no gradient.  The guard may cover at most 1 % of the pixels.  Stripes
of zero upstream gradient are added on purpose (live pixels with zero dL/dC).  At every unguarded pixel the HIP forward's
alphas (atol 1e-5) and last_ids (exactly) -- where the v1 / v2 kernels start their walk -- are checked against the oracle's.

Bars: those of test_hip_backward.py::test_raster_backward_vs_autograd (tests/helpers.py::assert_grad_close): max norm
2e-3 and 2e-3 per element with |g_ref| >= 1e-3 max|g_ref|.
"""
import numpy as np
import pytest
import torch

import oracle
from helpers import assert_grad_close, np_, oracle_project, raster_scene, simple_camera
from mojosplat_amd import Camera, _hip
from mojosplat_amd.autograd import project_gaussians_autograd, rasterize_gaussians_autograd, render_gaussians_trainable
from mojosplat_amd.binning import bin_gaussians_to_tiles_hip
from mojosplat_amd.projection import EPS2D, project_gaussians_hip
from mojosplat_amd.rasterization import rasterize_gaussians_hip
from mojosplat_amd.scenes import randscene_v1
from mojosplat_amd.utils import look_at
from oracle import torch_oracle

pytestmark = pytest.mark.gpu

ELEM_F64 = 2e-3          # as test_hip_backward.py
MARGIN_EPS = 1e-5        # branch guard
GUARD_CAP = 0.01         # at most this fraction of the pixels guarded
RASTER_NAMES = ("means2d", "conics", "colors", "opacities")


def _kernel_name(C, workspace=True):
    """Which kernel ms::rasterize_bwd launches (rasterize_bwd.hip:597-679)."""
    if C <= 4 and workspace:
        return "v2<3>" if C <= 3 else "v2<4>"
    return f"v1<{3 if C <= 3 else 4 if C <= 4 else 8 if C <= 8 else 16 if C <= 16 else 32}>"


# ------------------------------------------------------------------ fixtures (CPU, identical bytes everywhere)
class Scene2D:
    """A projected + binned scene (C oracle) on an H x W image at tile size ts."""

    def __init__(self, N, W, H, ts, C, seed, *, f=None, depth_range=(1.5, 5.0), scale_log=-2.0,
                 opacity_range=(0.5, 0.95), spread=1.0, snap=0):
        means3d, ls, quats, op, colors = raster_scene(N, seed=seed, depth_range=depth_range, scale_log=scale_log,
                                                      opacity_range=opacity_range, channels=C)
        means3d[:, :2] *= spread
        cam = simple_camera(H=H, W=W, f=f or 0.9 * W)
        if snap:
            # the `snap` nearest Gaussians: centres on pixel centres, opacity in [0.9995, 1]: alpha is clamped to 0.999 there
            g = torch.Generator().manual_seed(seed + 1)
            near = torch.argsort(means3d[:, 2])[:snap]
            z = means3d[near, 2]
            px = torch.randint(2, W - 2, (snap,), generator=g).float() + 0.5
            py = torch.randint(2, H - 2, (snap,), generator=g).float() + 0.5
            means3d[near, 0] = (px - cam.cx) * z / cam.fx
            means3d[near, 1] = (py - cam.cy) * z / cam.fy
            op[near] = 0.9995 + 0.0005 * torch.rand(snap, generator=g)
        self.m2, self.con, dep, rad = oracle_project(oracle, means3d, ls, quats, op, cam)
        self.ids, self.ranges = oracle.bin_tiles(self.m2, rad, dep, H, W, ts)
        self.col, self.op = np_(colors), np_(op)
        self.N, self.C, self.W, self.H, self.ts = N, C, W, H, ts
        assert self.ids.size > 0

    def camera(self, device):
        return simple_camera(device, H=self.H, W=self.W)


def _regime(m2, con, op, ranges, ids, H, W, ts):
    """The float64 walk of torch_oracle.rasterize, per pixel: did it terminate (T(1 - alpha) <= 1e-4), how many blended
    pairs sit in the 0.999 clamp, and how close any blended pair's unclamped alpha came to 0.999 (relative)."""
    m2, con, op = (np.asarray(a, np.float64) for a in (m2, con, op))
    term = np.zeros((H, W), bool)
    nclamp = np.zeros((H, W), np.int64)
    cmargin = np.full((H, W), np.inf)
    th, tw = ranges.shape[:2]
    for ty in range(th):
        for tx in range(tw):
            s, e = ranges[ty, tx]
            y0, x0 = ty * ts, tx * ts
            y1, x1 = min(y0 + ts, H), min(x0 + ts, W)
            if e <= s or y1 <= y0 or x1 <= x0:
                continue
            py, px = np.meshgrid(np.arange(y0, y1) + 0.5, np.arange(x0, x1) + 0.5, indexing="ij")
            g = ids[s:e]
            dx = m2[g, 0][:, None] - px.reshape(1, -1)
            dy = m2[g, 1][:, None] - py.reshape(1, -1)
            sigma = 0.5 * (con[g, 0][:, None] * dx * dx + con[g, 2][:, None] * dy * dy) + con[g, 1][:, None] * dx * dy
            ov = op[g][:, None] * np.exp(-sigma)
            alpha = np.minimum(ov, 0.999)
            mask = (sigma >= 0) & (alpha >= 1.0 / 255.0)
            Tn = np.cumprod(1.0 - np.where(mask, alpha, 0.0), axis=0)
            live = mask & (Tn > 1e-4)
            shape = (y1 - y0, x1 - x0)
            term[y0:y1, x0:x1] = (mask & ~live).any(0).reshape(shape)
            nclamp[y0:y1, x0:x1] = (live & (ov > 0.999)).sum(0).reshape(shape)
            cmargin[y0:y1, x0:x1] = np.where(live, np.abs(ov / 0.999 - 1.0), np.inf).min(0).reshape(shape)
    lens = (ranges[..., 1] - ranges[..., 0]).reshape(-1)
    return dict(terminated=term, clamped=nclamp, clamp_margin=cmargin, max_list=int(lens.max()))


class Upstream:
    """Upstream gradients with the branch guard applied (see the module docstring)."""

    def __init__(self, m2, con, col, op, bg, ranges, ids, H, W, ts, seed, with_alpha=False):
        C = col.shape[1]
        o_img, o_alph, o_last, margin = oracle.rasterize_fwd(m2, con, col, op, None if bg is None else np_(bg),
                                                             ranges, ids, H, W, ts, margin=True)
        self.regime = _regime(m2, con, op, ranges, ids, H, W, ts)
        self.guard = (margin < MARGIN_EPS) | (self.regime["clamp_margin"] < MARGIN_EPS)
        assert self.guard.mean() <= GUARD_CAP, f"branch guard covers {self.guard.mean():.2%} of the pixels"
        g = torch.Generator().manual_seed(seed)
        v_img = torch.rand(H, W, C, generator=g) * 2.0 - 0.6
        v_img[1::5] = 0.0                 # stripes: live pixels with zero dL/dC
        v_img[:, 3::7] = 0.0
        keep = torch.from_numpy(~self.guard)
        self.v_img = v_img * keep[..., None]
        self.v_a = (torch.rand(H, W, generator=g) - 0.5) * keep if with_alpha else None
        self.o_alph, self.o_last = o_alph, o_last

    def check_forward(self, alphas, last, tag):
        """The HIP forward's alphas / last_ids against the oracle's at every unguarded pixel."""
        keep = ~self.guard
        a, l = np_(alphas), np_(last)
        assert np.abs(a - self.o_alph)[keep].max() <= 1e-5, f"{tag}: alphas"
        assert (l == self.o_last)[keep].all(), f"{tag}: last_ids differ at {int((l != self.o_last)[keep].sum())} px"


def _raster_ref(m2, con, col, op, bg, ranges, ids, H, W, ts, up):
    """float64 autograd of torch_oracle.rasterize -> (image, alphas, [grads of means2d, conics, colours, opacities], v_bg)."""
    rl = [torch.from_numpy(np.asarray(a)).double().requires_grad_(True) for a in (m2, con, col, op)]
    rbg = None if bg is None else bg.detach().cpu().double().requires_grad_(True)
    rimg, ralph = torch_oracle.rasterize(*rl, rbg, torch.from_numpy(ranges), torch.from_numpy(ids), H, W, ts)
    loss = (rimg * up.v_img.double()).sum()
    if up.v_a is not None:
        loss = loss + (ralph * up.v_a.double()).sum()
    loss.backward()
    return rimg.detach(), ralph.detach(), [t.grad for t in rl], None if rbg is None else rbg.grad


def _background(C, seed, device=None):
    return (torch.rand(C, generator=torch.Generator().manual_seed(seed)) * 0.6 + 0.1).to(device or "cpu")


# ------------------------------------------------------------------ 1. per-stage matrix
@pytest.mark.parametrize("ts", [8, 16, 24, 32])
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 8, 16, 32])
def test_per_stage_backward_every_channel_count_and_tile_size(device, C, ts):
    """rasterize_gaussians_autograd (_RasterizeHip: ms_rasterize_to_pixels_3dgs_bwd with ms_rasterize_bwd_workspace_bytes)
    on a ragged 88 x 60 image (a multiple of none of 16 / 24 / 32, ragged at 8: the 16-px sub-blocks of ts 24 / 32 hang over
    the tile's edge and the image's).  Reaches k_rasterize_bwd_v2<3,4,false> for C = 1, 2, 3 (C = 1, 2 never ran before),
    k_rasterize_bwd_v2<4,4,false> for C = 4 and the one-atomic-per-component k_rasterize_bwd<8|16|32> for C = 5..32 (never
    executed before), each followed by k_unpack_grads<true> on the packed path.  Background gradient included."""
    sc = Scene2D(150, 88, 60, ts, C, seed=31)
    bg = _background(C, 5 + C)
    up = Upstream(sc.m2, sc.con, sc.col, sc.op, bg, sc.ranges, sc.ids, sc.H, sc.W, ts, seed=C * 10 + ts)
    to = lambda a: torch.from_numpy(np.asarray(a)).to(device)
    cam = sc.camera(device)
    with torch.no_grad():
        _, alphas, last = rasterize_gaussians_hip(to(sc.m2), to(sc.con), to(sc.col), to(sc.op), bg.to(device),
                                                  to(sc.ranges), to(sc.ids), cam, ts, return_aux=True)
    up.check_forward(alphas, last, f"C{C}/ts{ts}")
    leaves = [to(a).requires_grad_(True) for a in (sc.m2, sc.con, sc.col, sc.op)]
    bgd = bg.to(device).requires_grad_(True)
    img = rasterize_gaussians_autograd(*leaves, bgd, to(sc.ranges), to(sc.ids), cam, ts)
    (img * up.v_img.to(device)).sum().backward()
    rimg, _, rgrads, rbg = _raster_ref(sc.m2, sc.con, sc.col, sc.op, bg, sc.ranges, sc.ids, sc.H, sc.W, ts, up)
    assert np.abs(np_(img) - rimg.numpy())[~up.guard].max() <= 1e-4
    tag = f"{_kernel_name(C)}/C{C}/ts{ts}"
    for name, a, b in zip(RASTER_NAMES, leaves, rgrads):
        assert_grad_close(f"{tag}/{name}", a.grad, b, elem_rel=ELEM_F64)
    assert_grad_close(f"{tag}/background", bgd.grad, rbg, elem_rel=ELEM_F64)


# ------------------------------------------------------------------ 2. the C-ABI entry point directly
def _abi_bwd(L, dev, sc, alphas, last, bg, v_img, v_a, ws_kind, overwrite, prefill):
    """One ms_rasterize_to_pixels_3dgs_bwd call; prefill = the four output tensors' contents before it."""
    to = lambda a: torch.from_numpy(np.asarray(a)).to(dev)
    m2, con, col, op = (to(a).contiguous() for a in (sc.m2, sc.con, sc.col, sc.op))
    outs = [p.clone().to(dev) for p in prefill]
    N, C = sc.N, sc.C
    if ws_kind == "none":
        ws, nbytes = None, 0
    elif ws_kind == "rows":   # packed rows, no room for the heaviest-first order
        nbytes = N * 64
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        nbytes = L.ms_rasterize_bwd_workspace_bytes(N, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    ranges, ids = to(sc.ranges), to(sc.ids)
    vimg = v_img.to(dev).contiguous()
    va = None if v_a is None else v_a.to(dev).contiguous()
    bgd = None if bg is None else bg.to(dev).contiguous()
    with torch.cuda.device(dev):
        _hip.check(L.ms_rasterize_to_pixels_3dgs_bwd(
            N, ids.numel(), _hip.ptr(m2), _hip.ptr(con), _hip.ptr(col), C, _hip.ptr(op), _hip.ptr(bgd), sc.W, sc.H, sc.ts,
            _hip.ptr(ranges), _hip.ptr(ids), _hip.ptr(alphas), _hip.ptr(last), _hip.ptr(vimg), _hip.ptr(va),
            *[_hip.ptr(o) for o in outs], _hip.ptr(ws), nbytes, overwrite, _hip.stream(dev)), "ms_rasterize_to_pixels_3dgs_bwd")
    torch.cuda.synchronize(dev)
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("C", [2, 3, 4, 8])
def test_abi_backward_workspaces_overwrite_and_alpha_gradients(device, C):
    """ms_rasterize_to_pixels_3dgs_bwd called directly (via _hip.lib()), on 96 x 72 at ts 16:
    * workspace None (k_rasterize_bwd<3|4|8> even for C <= 4), exactly N * 64 bytes (packed rows, k_rasterize_bwd_v2 in image
      order: no room for k_bwd_order's heaviest-first order) and ms_rasterize_bwd_workspace_bytes (v2 heaviest first);
    * overwrite = 1 on outputs pre-filled with NaN (must ignore them: the memset of the v1 path, k_unpack_grads<true>) and
      overwrite = 0 on outputs pre-filled with random values (must add: v1's atomics, k_unpack_grads<false>), checked as
      result - prefill;
    * v_render_alphas non-NULL (the loss gains (alphas * v_a).sum(); read by every kernel, NULL everywhere else in the
      suite), with and without a background, and NULL with a background."""
    L = _hip.lib()
    sc = Scene2D(160, 96, 72, 16, C, seed=41)
    bgc = _background(C, 77)
    g = torch.Generator().manual_seed(9)
    for bg, with_alpha in ((None, True), (bgc, True), (bgc, False)):
        up = Upstream(sc.m2, sc.con, sc.col, sc.op, bg, sc.ranges, sc.ids, sc.H, sc.W, 16, seed=C + 3 * with_alpha,
                      with_alpha=with_alpha)
        to = lambda a: torch.from_numpy(np.asarray(a)).to(device)
        with torch.no_grad():
            _, alphas, last = rasterize_gaussians_hip(to(sc.m2), to(sc.con), to(sc.col), to(sc.op),
                                                      None if bg is None else bg.to(device), to(sc.ranges), to(sc.ids),
                                                      sc.camera(device), 16, return_aux=True)
        up.check_forward(alphas, last, f"C{C}")
        _, _, rgrads, _ = _raster_ref(sc.m2, sc.con, sc.col, sc.op, bg, sc.ranges, sc.ids, sc.H, sc.W, 16, up)
        for ws_kind in ("none", "rows", "full"):
            kern = _kernel_name(C, ws_kind != "none")
            for overwrite in (1, 0):
                if overwrite:
                    prefill = [torch.full_like(r, float("nan"), dtype=torch.float32) for r in rgrads]
                else:   # of the gradient's own size: result - prefill keeps the gradient's fp32 precision
                    prefill = [((torch.rand(r.shape, generator=g) * 2 - 1) * r.abs().max()).float() for r in rgrads]
                got = _abi_bwd(L, device, sc, alphas, last, bg, up.v_img, up.v_a, ws_kind, overwrite, prefill)
                tag = f"{kern}/ws={ws_kind}/overwrite={overwrite}/C{C}/bg={bg is not None}/v_alpha={with_alpha}"
                for name, o, p, r in zip(RASTER_NAMES, got, prefill, rgrads):
                    assert torch.isfinite(o).all(), f"{tag}/{name}"
                    res = o if overwrite else o.double() - p.double()
                    assert_grad_close(f"{tag}/{name}", res, r, elem_rel=ELEM_F64)


# ------------------------------------------------------------------ 3. long and saturated lists
# The saturated scene's bar against exact float64.  The v1 / v2 kernels take T_final = 1 - render_alphas (the gsplat ABI),
# and alphas near 1 stored in fp32 carry 2^-25 absolute, i.e. up to 3e-4 relative in a T_final of 1e-4.  Every gradient term
# of a pixel is proportional to its T_final, so this is the same as scaling the pixel's upstream gradient by (1 + delta);
# summed over pixels whose terms nearly cancel it reaches (measured, seed below; float64 emulation of the storage alone
# gives the same numbers on the same elements) 6.8e-3 on a conic and 2.9e-3 on a mean.  The kernels' own arithmetic is held
# to ELEM_F64 against the float64 reference whose upstream carries that storage delta (see _per_stage_vs_f64).
SATURATED_F64 = 1.5e-2


class _Scaled:
    def __init__(self, v_img, v_a):
        self.v_img, self.v_a = v_img, v_a


def _per_stage_vs_f64(device, sc, bg, seed, tag, saturated=False):
    up = Upstream(sc.m2, sc.con, sc.col, sc.op, bg, sc.ranges, sc.ids, sc.H, sc.W, sc.ts, seed=seed)
    to = lambda a: torch.from_numpy(np.asarray(a)).to(device)
    cam = sc.camera(device)
    with torch.no_grad():
        _, alphas, last = rasterize_gaussians_hip(to(sc.m2), to(sc.con), to(sc.col), to(sc.op), bg.to(device),
                                                  to(sc.ranges), to(sc.ids), cam, sc.ts, return_aux=True)
    up.check_forward(alphas, last, tag)
    leaves = [to(a).requires_grad_(True) for a in (sc.m2, sc.con, sc.col, sc.op)]
    bgd = bg.to(device).requires_grad_(True)
    img = rasterize_gaussians_autograd(*leaves, bgd, to(sc.ranges), to(sc.ids), cam, sc.ts)
    (img * up.v_img.to(device)).sum().backward()
    _, ralph, rgrads, rbg = _raster_ref(sc.m2, sc.con, sc.col, sc.op, bg, sc.ranges, sc.ids, sc.H, sc.W, sc.ts, up)
    bar = SATURATED_F64 if saturated else ELEM_F64
    for name, a, b in zip(RASTER_NAMES, leaves, rgrads):
        assert_grad_close(f"{tag}/{name}", a.grad, b, elem_rel=bar)
    assert_grad_close(f"{tag}/background", bgd.grad, rbg, elem_rel=bar)
    if saturated:
        # the float64 gradient of a kernel that gets T_final from fp32 alphas exactly: each pixel's upstream scaled by
        # T_stored / T_final, T_stored = 1 - fp32(1 - T_final)
        Tt = 1.0 - ralph.numpy()
        Ts = 1.0 - (1.0 - Tt).astype(np.float32).astype(np.float64)
        delta = torch.from_numpy(Ts / np.where(Tt > 0, Tt, 1.0))
        sc_up = _Scaled(up.v_img.double() * delta[..., None], None)
        _, _, sgrads, sbg = _raster_ref(sc.m2, sc.con, sc.col, sc.op, bg, sc.ranges, sc.ids, sc.H, sc.W, sc.ts, sc_up)
        for name, a, b in zip(RASTER_NAMES, leaves, sgrads):
            assert_grad_close(f"{tag}/alphas-in-fp32/{name}", a.grad, b, elem_rel=ELEM_F64)
        assert_grad_close(f"{tag}/alphas-in-fp32/background", bgd.grad, sbg, elem_rel=ELEM_F64)
    return up.regime


@pytest.mark.parametrize("C", [3, 8])
def test_per_stage_backward_long_lists(device, C):
    """Tiles with several hundred entries of faint Gaussians (opacity 0.05-0.2: the pixels do not saturate): k_rasterize_bwd
    v1 (C = 8) walks them in several 256-entry b0 batches, k_rasterize_bwd_v2<3,4,false> (C = 3) in many kBatch = 64 rounds.
    The fixture must keep its regime: a list longer than 2 x 256 entries, no pixel terminated early."""
    sc = Scene2D(1200, 64, 48, 16, C, seed=7, f=60, scale_log=-2.3, opacity_range=(0.05, 0.2), spread=0.5)
    regime = _per_stage_vs_f64(device, sc, _background(C, 3), 50 + C, f"{_kernel_name(C)}/long/C{C}")
    assert regime["max_list"] > 2 * 256, regime["max_list"]
    assert not regime["terminated"].any()


@pytest.mark.parametrize("C", [3, 8])
def test_per_stage_backward_saturated_pixels(device, C):
    """A dense opaque scene (opacity 0.95-1.0, the 40 nearest Gaussians centred on pixel centres with opacity >= 0.9995):
    most pixels terminate at T <= 1e-4, and the pixels under those centres blend them through the 0.999 clamp, which has no
    geometry gradient.  k_rasterize_bwd_v2<3,4,false> (C = 3) and k_rasterize_bwd<8> (C = 8) recover T back to front by
    dividing out alphas up to 0.999 from T_final = 1 - render_alphas.
    Measured elem_rel_max against exact float64: C = 3 conics 6.8e-3, means2d 1.3e-3; C = 8 means2d 2.9e-3 -- all of it the
    fp32 storage of alphas near 1 (SATURATED_F64); against float64 with that storage emulated the kernels stay within
    ELEM_F64.  Regime: >= 1/3 of the pixels terminate early (1823 of 3072), >= 20 clamped blended pairs (27), a list of
    more than 256 entries (430)."""
    sc = Scene2D(600, 64, 48, 16, C, seed=8, scale_log=-2.0, opacity_range=(0.95, 1.0), spread=0.6, snap=40)
    regime = _per_stage_vs_f64(device, sc, _background(C, 4), 60 + C, f"{_kernel_name(C)}/saturated/C{C}", saturated=True)
    assert regime["terminated"].sum() >= sc.H * sc.W // 3, int(regime["terminated"].sum())
    assert regime["clamped"].sum() >= 20, int(regime["clamped"].sum())
    assert regime["max_list"] > 256


# ------------------------------------------------------------------ 4. the fused differentiable frame
FUSED_CASES = [(1, 16, "v2<3,4,false> + k_project_ewa_bwd<1>"), (4, 16, "v2<4,4,false> + k_project_ewa_bwd<1>"),
               (8, 16, "non-packed: memset + v1<8> + ms_project_gaussians_bwd"),
               (32, 16, "non-packed: memset + v1<32> + ms_project_gaussians_bwd"),
               (3, 8, "v2<3,4,true> (records) + k_project_ewa_bwd<1>"), (3, 24, "v2<3,4,true> (records) + k_project_ewa_bwd<1>")]


def _fused_vs_f64(device, C, ts, seed, half=False, tag=""):
    sc, cam = randscene_v1(300, 96, 64, ell=-2.5, seed=seed, device=device, channels=C)
    names = ("means3d", "scales", "quats", "opacities", "features")
    if half:
        sc["features"] = sc["features"].half()
    leaves = [sc[k].clone().requires_grad_(True) for k in names]
    bg = _background(C, seed, device).requires_grad_(True)
    H, W = cam.H, cam.W
    th, tw = -(-H // ts), -(-W // ts)
    # the reference: the HIP forward's visibility and gsplat-exact binning, float64 projection + rasteriser
    with torch.no_grad():
        m2h, conh, deph, radh = project_gaussians_autograd(*[l.detach() for l in leaves[:4]], cam)
        ids, ranges = bin_gaussians_to_tiles_hip(m2h, radh, deph, ts, tw, th)
    ids_c, ranges_c = np_(ids).astype(np.int32), np_(ranges).astype(np.int32)
    feats32 = np_(leaves[4].float())
    up = Upstream(np_(m2h), np_(conh), feats32, np_(leaves[3]), bg.detach(), ranges_c, ids_c, H, W, ts, seed=seed + 1)
    img = render_gaussians_trainable(*leaves, cam, background_color=bg, tile_size=ts)
    img.backward(up.v_img.to(device))
    rl = [l.detach().cpu().double().requires_grad_(True) for l in leaves]   # (fp16 features: the rounded values, exactly)
    rbg = bg.detach().cpu().double().requires_grad_(True)
    vm = cam.view_matrix.double().cpu()
    rm2, rcon, _ = torch_oracle.project(rl[0], rl[1], rl[2], vm, cam.fx, cam.fy, cam.cx, cam.cy, W, H)
    rimg, _ = torch_oracle.rasterize(rm2, rcon, rl[4], rl[3], rbg, torch.from_numpy(ranges_c), torch.from_numpy(ids_c), H, W, ts)
    keep = ~up.guard
    assert np.abs(np_(img) - rimg.detach().numpy())[keep].max() <= 2e-4
    (rimg * up.v_img.double()).sum().backward()
    return names, leaves, rl, bg, rbg


@pytest.mark.parametrize("C,ts,path", FUSED_CASES)
def test_fused_frame_backward_vs_f64(device, C, ts, path):
    """render_gaussians_trainable with default arguments (the one-call differentiable frame, ms_render_bwd) against float64
    autograd of torch_oracle.project + rasterize on the HIP forward's visibility and binning (as
    test_end_to_end_gradients_and_finite_difference does for the quad-wave kernel).  C = 1, 4 at ts 16: the packed
    k_rasterize_bwd_v2<3|4,4,false> rows finished by k_project_ewa_bwd<1>; C = 8, 32 at ts 16: ms_render_bwd's non-packed
    branch (memset, k_rasterize_bwd<8|32>, then ms_project_gaussians_bwd with the frame's radii) -- never executed before;
    C = 3 at ts 8 / 24: k_rasterize_bwd_v2<3,4,true>, staged from the frame's ready-made records."""
    names, leaves, rl, bg, rbg = _fused_vs_f64(device, C, ts, seed=20 + C + ts)
    tag = f"fused/{path}/C{C}/ts{ts}"
    for name, a, b in zip(names, leaves, rl):
        assert_grad_close(f"{tag}/{name}", a.grad, b.grad, rel=5e-3, elem_rel=ELEM_F64)
    assert_grad_close(f"{tag}/background", bg.grad, rbg.grad, elem_rel=ELEM_F64)


# fp16 rounding of the returned colour gradient: relative 2^-11 on every element (all checked elements are fp16 normals)
FP16_OUT = 2.0 ** -11


def test_fp16_features_backward_vs_f64(device):
    """fp16 features through render_gaussians_trainable: the per-stage path (_RasterizeHip on fp32 copies,
    k_rasterize_bwd_v2<3,4,false>), the colour gradient cast back to fp16 by autograd.  Against float64 on the fp16-rounded
    features; the colour bar is widened by fp16's output rounding (2^-11 relative) only."""
    names, leaves, rl, bg, rbg = _fused_vs_f64(device, 3, 16, seed=90, half=True)
    assert leaves[4].grad.dtype == torch.float16
    for name, a, b in zip(names, leaves, rl):
        widen = FP16_OUT if a.dtype == torch.float16 else 0.0
        assert_grad_close(f"fp16/per-stage v2<3>/{name}", a.grad.float(), b.grad, rel=5e-3 + widen, elem_rel=ELEM_F64 + widen)
    assert_grad_close("fp16/per-stage v2<3>/background", bg.grad, rbg.grad, elem_rel=ELEM_F64)


# ------------------------------------------------------------------ 5. the projection backward through the ABI
def test_projection_backward_linear_scales_rotated_camera_through_the_abi(device):
    """ms_project_gaussians_bwd (k_project_ewa_bwd<0>) with scales_are_log = 0 and v_depths = NULL under a rotated look_at
    camera -- the float64 test of this entry point so far used R = I and log scales.  Gaussians culled by the near plane or
    off-screen get exactly zero gradients; v_depths = NULL equals v_depths zero-filled bit for bit; a non-NULL v_depths is
    checked too."""
    L = _hip.lib()
    N = 240
    g = torch.Generator().manual_seed(12)
    eye, target = torch.tensor([2.5, -1.5, 4.0]), torch.tensor([0.2, 0.1, 0.0])
    vm = look_at(eye, target, torch.tensor([0.0, 1.0, 0.0]))
    R, t = vm[:3, :3], vm[:3, 3]
    cam = Camera(R=R.contiguous().to(device), T=t.contiguous().to(device), H=64, W=96, fx=70.0, fy=72.0, cx=47.0,
                 cy=33.0, near=0.1, far=100.0)
    # camera-space positions, then to world: in view, behind / inside the near plane, and far off-screen
    pc = torch.randn(N, 3, generator=g) * torch.tensor([1.0, 0.7, 0.8]) + torch.tensor([0.0, 0.0, 4.0])
    pc[:20, 2] = torch.rand(20, generator=g) * 0.15 - 0.1          # z < near (0.1)
    pc[20:40, 0] = 40.0 * torch.sign(torch.randn(20, generator=g))  # off-screen
    means3d = ((pc - t) @ R).float()
    scales = torch.rand(N, 3, generator=g) * 0.25 + 0.03           # LINEAR scales
    quats = torch.randn(N, 4, generator=g) * 1.3                    # un-normalised
    opac = torch.rand(N, generator=g) * 0.8 + 0.15
    dm, ds, dq = (x.to(device).contiguous() for x in (means3d, scales, quats))
    _, _, _, rad = project_gaussians_hip(dm, ds, dq, opac.to(device), cam, scales_are_log=False)
    vis = (rad > 0).all(1).cpu()
    assert not vis[:40].any(), "the near-plane / off-screen Gaussians must be culled"
    assert vis.sum() >= N // 2
    wm, wc, wd = torch.randn(N, 2, generator=g), torch.randn(N, 3, generator=g), torch.randn(N, generator=g)
    vmf = cam._viewmat_f32().to(device)

    def call(v_depths):
        outs = [torch.full((N, k), float("nan"), device=device) for k in (3, 3, 4)]
        vmd, vcd = wm.to(device).contiguous(), wc.to(device).contiguous()
        vdd = None if v_depths is None else v_depths.to(device).contiguous()
        with torch.cuda.device(device):
            _hip.check(L.ms_project_gaussians_bwd(N, _hip.ptr(dm), _hip.ptr(ds), 0, _hip.ptr(dq), _hip.ptr(vmf), cam.fx, cam.fy,
                                                  cam.cx, cam.cy, cam.W, cam.H, EPS2D, _hip.ptr(rad), _hip.ptr(vmd), _hip.ptr(vcd),
                                                  _hip.ptr(vdd), *[_hip.ptr(o) for o in outs], _hip.stream(device)),
                       "ms_project_gaussians_bwd")
        return [o.cpu() for o in outs]

    got_null, got_zero, got_d = call(None), call(torch.zeros(N)), call(wd)
    for a, b in zip(got_null, got_zero):
        assert torch.equal(a, b)
    for with_depth, got in ((False, got_null), (True, got_d)):
        rl = [x.double().requires_grad_(True) for x in (means3d, scales, quats)]
        rm2, rcon, rdep = torch_oracle.project(*[x[vis] for x in rl], vm.double(), cam.fx, cam.fy, cam.cx, cam.cy, cam.W,
                                               cam.H, scales_are_log=False)
        loss = (rm2 * wm[vis]).sum() + (rcon * wc[vis]).sum()
        if with_depth:
            loss = loss + (rdep * wd[vis]).sum()
        loss.backward()
        for name, a, b in zip(("means3d", "scales", "quats"), got, rl):
            assert (a[~vis] == 0).all(), f"{name}: culled Gaussians must get zero gradients"
            assert_grad_close(f"project_bwd/linear/v_depths={'set' if with_depth else 'NULL'}/{name}", a, b.grad,
                              rel=1e-3, elem_rel=ELEM_F64)
