"""GPU: tight binning (reach_mask, csrc/binning.hip) and the quad reach test (csrc/rasterize.hip, make_raster_record) on
needle and edge-on disc Gaussians, held to the float64 references of tests/needle_cases.py -- the drop DECISIONS, which are
discrete, not a pixel bar ("Needles").  (a) the tight tile lists lie between the lower and upper sets of the
sandwich; (b) single-needle frames obey rule P on every path -- the one check that sees a quad dropped by the fused AND the
per-stage path, which share the test; (c) a scene of overlapping needles is the same frame on every path, bit for bit;
(d) the gradients that are linear in alpha."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import mojosplat_amd as ms
import needle_cases as nc
from helpers import PARITY_LOG, np_
from mojosplat_amd import _fused, _hip
from mojosplat_amd.autograd import rasterize_gaussians_autograd, render_gaussians_trainable
from mojosplat_amd.binning import bin_gaussians_to_tiles_hip

pytestmark = pytest.mark.gpu

STATS_LOG = os.path.join(os.path.dirname(PARITY_LOG), "needle_stats.jsonl")      # beside the parity counts
EPS2D = 0.3
TIGHT, BLOCK_MASKS = 1, 4       # bits of ms_project_isect_count's `tight` word (include/mojosplat_hip.h)


def _record(**rec):
    line = json.dumps(rec)
    print("NEEDLES", line)
    try:
        os.makedirs(os.path.dirname(STATS_LOG), exist_ok=True)
        with open(STATS_LOG, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def _to(sc, device):
    return {k: v.to(device) for k, v in sc.items()}


def _args(sc):
    return sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], sc["features"]


# ------------------------------------------------------------------ (a) tight lists
def hip_tight_lists(sc, cam, ts, tight, row_range=None, scales_are_log=True):
    """ms_project_isect_count(tight) + ms_isect_tiles_emit(tight, lazy = 0) through the C ABI, as the header describes the
    pair: the projected arrays of that call, the emitted words, the tile ranges and the size record (all on the host)."""
    L = _hip.lib()
    dev = sc["means3d"].device
    N = sc["means3d"].shape[0]
    tw, th = -(-cam.W // ts), -(-cam.H // ts)
    r0, r1 = (0, th) if row_range is None else row_range
    means3d, scales, quats = (_hip.f32c(sc[k]) for k in ("means3d", "scales", "quats"))
    opac = _hip.f32c(sc["opacities"].reshape(-1))
    vm = cam._viewmat_f32().to(dev)
    ws_bytes = L.ms_isect_workspace_bytes(N, tw, th)
    assert ws_bytes > 0
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    m2 = torch.empty((N, 2), dtype=torch.float32, device=dev)
    con = torch.empty((N, 3), dtype=torch.float32, device=dev)
    dep = torch.empty((N,), dtype=torch.float32, device=dev)
    rad = torch.empty((N, 2), dtype=torch.int32, device=dev)
    ranges = torch.zeros((th, tw, 2), dtype=torch.int32, device=dev)
    info = torch.zeros(8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _hip.stream(dev)
        _hip.check(L.ms_project_isect_count(
            N, _hip.ptr(means3d), _hip.ptr(scales), int(scales_are_log), _hip.ptr(quats), _hip.ptr(opac), _hip.ptr(vm),
            cam.fx, cam.fy, cam.cx, cam.cy, cam.W, cam.H, EPS2D, cam.near, cam.far, 0.0, ts, r0, r1, tight,
            _hip.ptr(m2), _hip.ptr(con), _hip.ptr(dep), _hip.ptr(rad), _hip.ptr(ws), ws.numel(), _hip.ptr(ranges),
            _hip.ptr(info), None, st), "ms_project_isect_count")
        torch.cuda.current_stream(dev).synchronize()
        host = [int(v) for v in info.cpu().tolist()]       # the device record, copied to the host
        M = host[0]
        assert 0 <= M <= N * tw * th
        words = torch.full((M,), -1, dtype=torch.int32, device=dev)
        if M > 0:
            keys = torch.empty(M, dtype=torch.int64, device=dev)
            tmp = torch.empty(M, dtype=torch.int64, device=dev) if host[4] > 0 else None
            _hip.check(L.ms_isect_tiles_emit(
                N, _hip.ptr(m2), _hip.ptr(rad), _hip.ptr(dep), ts, tw, th, r0, r1, _hip.ptr(ws), ws.numel(),
                _hip.ptr(ranges), (ctypes.c_int64 * 8)(*host), tight, 0, 0.0, 0.0, _hip.ptr(keys), _hip.ptr(tmp),
                _hip.ptr(words), None, st), "ms_isect_tiles_emit")
        torch.cuda.current_stream(dev).synchronize()
    return dict(m2=m2, con=con, dep=dep, rad=rad, words=np_(words), ranges=np_(ranges), info=host, M=M, tw=tw, th=th,
                band=(r0, r1))


def _check_ranges(t):
    """isect_info[0] and the ranges equal what was emitted: the band's tiles tile [0, M) in order, no tile outside the
    band holds anything, every slot was written."""
    r = t["ranges"].reshape(-1, 2).astype(np.int64)
    r0, r1 = t["band"]
    tw = t["tw"]
    inside = r[r0 * tw:r1 * tw]
    outside = np.concatenate([r[:r0 * tw], r[r1 * tw:]])
    assert (outside[:, 0] == outside[:, 1]).all()
    assert (inside[:, 0] <= inside[:, 1]).all()
    if len(inside):
        assert inside[0, 0] == 0 and inside[-1, 1] == t["M"] and (inside[1:, 0] == inside[:-1, 1]).all()
    else:
        assert t["M"] == 0
    assert len(t["words"]) == t["M"] and (t["words"] >= 0).all()


def _is_subsequence(sub, full):
    it = iter(full)
    return all(any(x == y for y in it) for x in sub)


def _sandwich_checks(t, ids, sc_cpu, meta, ts, tag, box_ids, box_ranges, ratio_cap=True):
    """The assertions of (a) for one pair of lists.  ids: the Gaussian of every emitted word."""
    N, tw, th = len(meta["family"]), t["tw"], t["th"]
    assert ((ids >= 0) & (ids < N)).all()
    for y in range(th):
        for x in range(tw):
            a, b = t["ranges"][y, x]
            c, d = box_ranges[y, x]
            # nothing invented, (depth, id) order kept
            assert _is_subsequence(ids[a:b].tolist(), box_ids[c:d].tolist()), (tag, x, y)
    T = nc.lists_to_pairs(ids, t["ranges"], N)
    B = nc.lists_to_pairs(box_ids, box_ranges, N)
    boxes = nc.tile_boxes(np_(t["m2"]), np_(t["rad"]), ts, tw, th, t["band"])
    assert (B == nc.box_pairs(boxes, tw, th)).all()      # the box lists are gsplat's boxes (and the host's restatement)
    L, U = nc.tile_sandwich(np_(t["m2"]), np_(t["con"]), np_(sc_cpu["opacities"]), boxes, ts, tw, th)
    n = B.reshape(N, -1).sum(1)
    masked = (n >= 2) & (n <= 64)
    missing, extra = L & ~T, T & ~U & masked[:, None, None]
    assert not missing.any(), (tag, "in L, not in the tight list", np.argwhere(missing)[:8].tolist())
    assert not extra.any(), (tag, "in the tight list, not in U", np.argwhere(extra)[:8].tolist())
    assert (T[~masked] == B[~masked]).all(), (tag, "a box of 1 or of more than 64 tiles is kept whole")
    stats = dict(tag=tag, pairs_box=int(B.sum()), pairs_tight=int(T.sum()), boxes_over_64=int((n > 64).sum()),
                 largest_masked_box=int(n[masked].max()) if masked.any() else 0)
    for name, f in (("needles", nc.NEEDLE), ("discs", nc.DISC), ("border", nc.BORDER)):
        m = meta["family"] == f
        if B[m].sum():
            stats[name + "_tight_over_box"] = round(float(T[m].sum() / B[m].sum()), 4)
            stats[name + "_tight_not_in_L"] = round(float((T[m] & ~L[m]).sum() / max(T[m].sum(), 1)), 4)
    _record(**stats)
    if ratio_cap:       # a mask that quietly became all ones is a failure
        assert stats["needles_tight_over_box"] <= 0.7, stats
    return T, B, L, U


LIST_CASES = [(8, False, True, None), (16, False, False, None), (32, False, True, None), (64, False, True, None),
              (16, True, True, None), (16, False, True, (3, 5)), (64, False, False, (2, 4))]


@pytest.mark.parametrize("ts,general,scales_log,band", LIST_CASES)
def test_tight_lists_lie_between_the_sandwich(device, ts, general, scales_log, band):
    sc_cpu, meta, cam = nc.needle_scene(ts, general=general, scales_log=scales_log)
    sc = _to(sc_cpu, device)
    t = hip_tight_lists(sc, cam, ts, TIGHT, band, scales_are_log=scales_log)
    _check_ranges(t)
    box_ids, box_ranges = bin_gaussians_to_tiles_hip(t["m2"], t["rad"], t["dep"], ts, t["tw"], t["th"], row_range=band)
    _sandwich_checks(t, t["words"], sc_cpu, meta, ts, f"tight ts={ts} general={general} log={scales_log} band={band}",
                     np_(box_ids), np_(box_ranges), ratio_cap=band is None)   # (inside a band through their means needles fill their boxes)


@pytest.mark.parametrize("ts", nc.TILE_SIZES)
def test_tight_lists_on_boxes_of_64_65_1_and_2_tiles(device, ts):
    """The mask's on/off edges: 64 tiles is masked, 65 and 1 are kept whole, 2 is the smallest masked box."""
    sc_cpu, meta, cam = nc.edge_scene(ts)
    t = hip_tight_lists(_to(sc_cpu, device), cam, ts, TIGHT)
    _check_ranges(t)
    box_ids, box_ranges = bin_gaussians_to_tiles_hip(t["m2"], t["rad"], t["dep"], ts, t["tw"], t["th"])
    T, B, L, U = _sandwich_checks(t, t["words"], sc_cpu, meta, ts, f"edge boxes ts={ts}", np_(box_ids), np_(box_ranges),
                                  ratio_cap=False)
    assert tuple(B.reshape(4, -1).sum(1)) == nc.EDGE_BOXES
    assert T[0].sum() <= 0.7 * 64 and T[1].sum() == 65 and T[2].sum() == 1 and T[3].sum() == 2


@pytest.mark.parametrize("ts", nc.TILE_SIZES)
def test_block_masks_lie_between_the_sandwich_on_the_half_tile_grid(device, ts):
    """Bits 0 | 2: every emitted word is id << 4 | blocks (include/mojosplat_hip.h); a set block bit keeps that half-tile
    cell's pair.  The cells are held to L and U computed on the half-tile grid: L always, U where the kernel keeps its
    mask per cell (boxes of at most 16 tiles); on larger boxes the mask is per tile and the bits are the gsplat box of
    the half-tile grid."""
    sc_cpu, meta, cam = nc.needle_scene(ts)
    t = hip_tight_lists(_to(sc_cpu, device), cam, ts, TIGHT | BLOCK_MASKS)
    _check_ranges(t)
    N, tw, th, hs = len(meta["family"]), t["tw"], t["th"], ts // 2
    ids, blocks = t["words"] >> 4, t["words"] & 15
    assert (blocks != 0).all()
    box_ids, box_ranges = bin_gaussians_to_tiles_hip(t["m2"], t["rad"], t["dep"], ts, tw, th)
    # tile level: the same sandwich as without the block bits
    T, B, L, U = _sandwich_checks(t, ids, sc_cpu, meta, ts, f"block masks ts={ts}, tiles", np_(box_ids), np_(box_ranges))
    # cell level
    C = np.zeros((N, 2 * th, 2 * tw), bool)
    for y in range(th):
        for x in range(tw):
            a, b = t["ranges"][y, x]
            for g, q in zip(ids[a:b], blocks[a:b]):
                for bit in range(4):
                    if (q >> bit) & 1:
                        C[g, 2 * y + (bit >> 1), 2 * x + (bit & 1)] = True
    cell_ids, cell_ranges = bin_gaussians_to_tiles_hip(t["m2"], t["rad"], t["dep"], hs, 2 * tw, 2 * th)
    Bc = nc.lists_to_pairs(np_(cell_ids), np_(cell_ranges), N)
    cboxes = nc.tile_boxes(np_(t["m2"]), np_(t["rad"]), hs, 2 * tw, 2 * th)
    assert (Bc == nc.box_pairs(cboxes, 2 * tw, 2 * th)).all()
    Lc, Uc = nc.tile_sandwich(np_(t["m2"]), np_(t["con"]), np_(sc_cpu["opacities"]), cboxes, hs, 2 * tw, 2 * th)
    n = B.reshape(N, -1).sum(1)
    per_cell = (n >= 1) & (n <= 16)
    assert not (C & ~Bc).any(), "a block bit outside the half-tile grid's box"
    assert not (Lc & ~C).any(), ("in L on the half-tile grid, bit not set", np.argwhere(Lc & ~C)[:8].tolist())
    extra = C & ~Uc & per_cell[:, None, None]
    assert not extra.any(), ("bit set, not in U on the half-tile grid", np.argwhere(extra)[:8].tolist())
    # boxes of more than 16 tiles: a kept tile carries every cell of the half-tile box
    whole = Bc & np.repeat(np.repeat(T, 2, 1), 2, 2)
    assert (C[~per_cell] == whole[~per_cell]).all()
    m = meta["family"] == nc.NEEDLE
    _record(tag=f"block masks ts={ts}, cells", cells_box=int(Bc.sum()), cells_kept=int(C.sum()),
            needles_cells_over_box=round(float(C[m].sum() / Bc[m].sum()), 4),
            cells_not_in_L=round(float((C & ~Lc).sum() / max(C.sum(), 1)), 4), boxes_per_cell=int(per_cell.sum()))
    assert C[m].sum() <= 0.7 * Bc[m].sum()


# ------------------------------------------------------------------ (b) rule P, (d) gradients: single needles
def _stagewise(sc, cam, bg):
    """test_hip_fused.stagewise's three calls, and the projection's outputs."""
    m2, con, dep, rad = ms.project_gaussians(sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], cam, backend="hip")
    ids, ranges = ms.bin_gaussians_to_tiles(m2, rad, dep, cam.H, cam.W, 16, backend="hip")
    if ids.numel() == 0:
        return torch.zeros(cam.H, cam.W, sc["features"].shape[1], device=m2.device), (m2, con, dep, rad, ids, ranges)
    img = ms.rasterize_gaussians(m2, con, sc["features"], sc["opacities"], bg, ranges, ids, cam, tile_size=16, backend="hip")
    return img, (m2, con, dep, rad, ids, ranges)


@pytest.mark.parametrize("ts", nc.TILE_SIZES)
def test_single_needle_frames_obey_rule_p_on_every_path(device, ts):
    scene, meta, cam = nc.needle_scene(ts)
    bg = torch.zeros(3, device=device)
    worst, worst_share, worst_case, blended, undecided = 0.0, 0.0, None, 0, 0
    for i in nc.single_cases(meta):
        sc = _to(nc.single_scene(scene, i), device)
        ref, (m2, con, *_) = _stagewise(sc, cam, bg)
        for b in (16, 32, 64):
            img = ms.render_gaussians(*_args(sc), cam, background_color=bg, tile_size=16, bin_size=b, backend="hip")
            assert torch.equal(img, ref), (ts, i, b, "fused frame != per-stage frame")
        frame = np_(ref)
        assert (frame[..., 0] == frame[..., 1]).all() and (frame[..., 0] == frame[..., 2]).all()
        o = float(sc["opacities"][0])
        la, S, e = nc.alpha_reference(np_(m2), np_(con), o, cam.H, cam.W)
        r = nc.rule_p(frame[..., 0], la[0], e[0], o)
        case = dict(ts=ts, i=i, opacity=o, theta=float(meta["theta"][i]), aspect=float(meta["aspect"][i]),
                    sigma_px=round(float(meta["sigma_px"][i]), 2), family=int(meta["family"][i]))
        print("NEEDLES case", json.dumps(dict(case, worst=round(r["worst"], 4), undecided=r["undecided"], blending=r["blending"])))
        assert not any(r["bad"].values()), (case, r["bad"])
        assert r["share"] <= nc.UNDECIDED_CAP, (case, r["undecided"], r["blending"])
        if r["worst"] > worst:
            worst, worst_case = r["worst"], case
        worst_share, blended, undecided = max(worst_share, r["share"]), blended + r["blending"], undecided + r["undecided"]
    _record(tag=f"rule P ts={ts}", worst_ratio=round(worst, 4), worst_case=worst_case, worst_undecided_share=worst_share,
            blending_pixels=blended, undecided_pixels=undecided)


def _grad_bars(v, la, e, o, und):
    """The reference sums and their bars for one single-needle frame: v (H, W, 3) upstream, la / e (H, W), und the undecided
    pixels.  alpha64 = 2^la on the blending pixels (o <= 0.99: the 0.999 clamp never binds, T = 1, pixel = alpha * colour).
      colors.grad[c] = sum_p v[p, c] alpha64,   opacities.grad = sum_p sum_c v[p, c] alpha64 / o
    bar = sum |v| alpha64 (ln 2 * e + 2^-20)   the exponent, and the blend's own roundings
        + sum over undecided pixels of |v| alpha64   either decision is allowed there
        + 2^-16 sum |v| alpha64   the backward's two-term bf16 tile (tests/helpers.py, gradient bars)."""
    blend = la >= nc.LOG2_THR
    a64 = np.where(blend, np.exp2(la), 0.0)
    a_any = np.exp2(la)
    v = v.astype(np.float64)
    ref_c = (v * a64[..., None]).sum((0, 1))
    av = np.abs(v)
    bar_c = (av * (a64 * (math.log(2.0) * e + 2.0 ** -20))[..., None]).sum((0, 1)) + (av * (a_any * und)[..., None]).sum((0, 1)) + \
        2.0 ** -16 * (av * a64[..., None]).sum((0, 1))
    return ref_c, bar_c, ref_c.sum() / o, bar_c.sum() / o


@pytest.mark.parametrize("ts", nc.TILE_SIZES)
def test_single_needle_gradients_linear_in_alpha(device, ts):
    scene, meta, cam = nc.needle_scene(ts)
    bg = torch.zeros(3, device=device)
    g = torch.Generator().manual_seed(ts)
    v_cpu = torch.randn(cam.H, cam.W, 3, generator=g)
    v = v_cpu.to(device)
    worst = dict(colors=0.0, opacities=0.0)
    checked = 0
    for i in nc.single_cases(meta):
        o = float(scene["opacities"][i])
        if not (1.0 / 255.0 <= o <= 0.99):
            continue
        sc = _to(nc.single_scene(scene, i), device)
        _, (m2, con, dep, rad, ids, ranges) = _stagewise(sc, cam, bg)
        la, S, e = nc.alpha_reference(np_(m2), np_(con), o, cam.H, cam.W)
        r = nc.rule_p(np.zeros((cam.H, cam.W)), la[0], e[0], o)
        ref_c, bar_c, ref_o, bar_o = _grad_bars(v_cpu.numpy(), la[0], e[0], o, r["undecided_mask"])
        for path in ("per-stage", "fused"):
            col = sc["features"].clone().requires_grad_(True)
            op = sc["opacities"].clone().requires_grad_(True)
            if path == "per-stage":
                img = rasterize_gaussians_autograd(m2, con, col, op, bg, ranges, ids, cam, 16)
            else:
                img = render_gaussians_trainable(sc["means3d"], sc["scales"], sc["quats"], op, col, cam, background_color=bg)
            (img * v).sum().backward()
            got_c, got_o = np_(col.grad).astype(np.float64)[0], float(op.grad[0])
            err_c, err_o = np.abs(got_c - ref_c), abs(got_o - ref_o)
            print("NEEDLES grad", json.dumps(dict(ts=ts, i=i, path=path, opacity=o, err_over_bar_colors=round(float((err_c / bar_c).max()), 4),
                                                  err_over_bar_opacity=round(err_o / bar_o, 4))))
            assert (err_c <= bar_c).all(), (ts, i, path, "colors.grad", got_c.tolist(), ref_c.tolist(), bar_c.tolist())
            assert err_o <= bar_o, (ts, i, path, "opacities.grad", got_o, ref_o, bar_o)
            worst["colors"] = max(worst["colors"], float((err_c / bar_c).max()))
            worst["opacities"] = max(worst["opacities"], err_o / bar_o)
        checked += 1
    assert checked >= 8
    _record(tag=f"gradients ts={ts}", cases=checked, worst_err_over_bar=worst)


# ------------------------------------------------------------------ (c) a scene of overlapping needles
@pytest.fixture(scope="module")
def cloud(device):
    from helpers import simple_camera
    cam = simple_camera(H=384, W=512, f=400.0)
    sc = _to(nc.needle_cloud(3000, cam, seed=5), device)
    bg = torch.tensor([0.1, 0.2, 0.3], device=device)
    ref, _ = _stagewise(sc, cam, bg)
    assert float((ref - bg).abs().max()) > 0.1
    return sc, cam, bg, ref


def test_needle_cloud_is_one_frame_on_every_grid(device, cloud):
    sc, cam, bg, ref = cloud
    grids = [dict(tile_size=8), dict(tile_size=16), dict(tile_size=32), dict(tile_size=16, bin_size=16),
             dict(tile_size=16, bin_size=32), dict(tile_size=16, bin_size=64)]
    for kw in grids:
        _fused._state.clear()
        for _ in range(2):      # the second frame reuses the first one's scratch (and may speculate on its size record)
            img = ms.render_gaussians(*_args(sc), cam, background_color=bg, backend="hip", **kw)
            assert torch.equal(img, ref), kw


def test_needle_cloud_from_three_row_bands(device, cloud):
    sc, cam, bg, ref = cloud
    th = cam.H // 16
    frame = torch.full((cam.H, cam.W, 3), -1.0, device=device)
    for band in ((0, 7), (7, 15), (15, th)):
        _fused.render_fwd_hip(*_args(sc), cam, bg, 16, row_range=band, out=frame)
    assert torch.equal(frame, ref)


def test_needle_cloud_with_fp16_colours(device, cloud):
    sc, cam, bg, _ = cloud
    sc16 = dict(sc, features=sc["features"].half())
    ref16, _ = _stagewise(sc16, cam, bg.half())
    for kw in (dict(), dict(bin_size=32), dict(bin_size=64)):
        img = ms.render_gaussians(*_args(sc16), cam, background_color=bg, backend="hip", **kw)
        assert img.dtype == torch.float32 and torch.equal(img, ref16), kw


def test_needle_cloud_trainable_forward_is_the_same_frame(device, cloud):
    """render_gaussians_trainable's forward -- the quad-list frame -- equals the per-stage frame bit for bit."""
    sc, cam, bg, ref = cloud
    leaves = [t.clone().requires_grad_(True) for t in _args(sc)]
    img = render_gaussians_trainable(*leaves, cam, background_color=bg)
    assert torch.equal(img.detach(), ref)
