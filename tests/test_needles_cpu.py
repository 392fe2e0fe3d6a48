"""The needle references alone (tests/needle_cases.py), on the CPU: a plain float32 rasteriser -- the C oracle's, the path
tests/test_oracle_golden.py uses -- stays inside rule P on the chosen cases, the undecided band is as thin as the GPU
test's cap needs, and the tile sandwich is a sandwich that bites (L inside U, L not empty, U well short of the box)."""
import numpy as np
import pytest

import needle_cases as nc
import oracle
from helpers import np_, oracle_project


def _project(sc, cam):
    return oracle_project(oracle, sc["means3d"], sc["scales"], sc["quats"], sc["opacities"], cam)


def _oracle_frame(sc, cam, proj):
    m2, con, dep, rad = proj
    ids, ranges = oracle.bin_tiles(m2, rad, dep, cam.H, cam.W, 16)
    if ids.size == 0:
        return np.zeros((cam.H, cam.W), np.float32)
    img, _, _ = oracle.rasterize_fwd(m2, con, np_(sc["features"]), np_(sc["opacities"]), np.zeros(3, np.float32), ranges, ids,
                                     cam.H, cam.W, 16)
    assert (img[..., 0] == img[..., 1]).all() and (img[..., 0] == img[..., 2]).all()
    return img[..., 0]


@pytest.mark.parametrize("ts", nc.TILE_SIZES)
def test_oracle_single_frames_obey_rule_p(ts):
    scene, meta, cam = nc.needle_scene(ts)
    worst, worst_share, blended = 0.0, 0.0, 0
    for i in nc.single_cases(meta):
        sc = nc.single_scene(scene, i)
        proj = _project(sc, cam)
        frame = _oracle_frame(sc, cam, proj)
        o = float(sc["opacities"][0])
        la, S, e = nc.alpha_reference(proj[0], proj[1], o, cam.H, cam.W)
        r = nc.rule_p(frame, la[0], e[0], o)
        assert not any(r["bad"].values()), (ts, i, {k: meta[k][i] for k in meta}, r["bad"])
        assert (r["blending"] > 0) == (o >= 1.0 / 255.0), (ts, i, r["blending"])
        assert r["share"] <= nc.UNDECIDED_CAP, (ts, i, r["undecided"], r["blending"])
        worst, worst_share, blended = max(worst, r["worst"]), max(worst_share, r["share"]), blended + r["blending"]
    print(f"NEEDLES oracle ts={ts}: worst |log2 pixel - la64| / (e + 2^-20) = {worst:.3f}, worst undecided share = "
          f"{worst_share:.2e}, blending pixels = {blended}")


def _sandwich(scene, cam, ts, row_range=None):
    m2, con, dep, rad = _project(scene, cam)
    tw, th = -(-cam.W // ts), -(-cam.H // ts)
    boxes = nc.tile_boxes(m2, rad, ts, tw, th, row_range)
    L, U = nc.tile_sandwich(m2, con, np_(scene["opacities"]), boxes, ts, tw, th)
    return boxes, nc.box_pairs(boxes, tw, th), L, U, rad


@pytest.mark.parametrize("ts,general,scales_log", [(8, False, True), (16, False, False), (32, False, True), (64, False, True),
                                                   (16, True, True)])
def test_sandwich_is_nested_nonempty_and_tight(ts, general, scales_log):
    scene, meta, cam = nc.needle_scene(ts, general=general, scales_log=scales_log)
    if not scales_log:      # the oracle front end takes log scales: the linear scene must be the same scene
        scene = dict(scene, scales=scene["scales"].log())
    boxes, box, L, U, rad = _sandwich(scene, cam, ts)
    assert not (L & ~U).any() and not (U & ~box).any()
    alive = (rad > 0).all(1)
    assert (alive == (meta["opacity"] >= 1.0 / 255.0)).all()       # only the 0.002s are culled (0.004 > 1/255)
    assert (L.reshape(len(L), -1).any(1) == alive).all()            # every live Gaussian must keep a tile
    ratio = {}
    for name, f in (("needles", nc.NEEDLE), ("discs", nc.DISC), ("border", nc.BORDER)):
        m = meta["family"] == f
        n_box, n_u, n_l = int(box[m].sum()), int(U[m].sum()), int(L[m].sum())
        ratio[name] = n_u / n_box
        print(f"NEEDLES sandwich ts={ts} general={general} {name}: box pairs {n_box}, U {n_u} ({n_u / n_box:.3f}), L {n_l} "
              f"({n_l / n_box:.3f}), largest box {int(box[m].reshape(int(m.sum()), -1).sum(1).max())} tiles")
    assert ratio["needles"] <= 0.7
    # a band through the needles: the boxes are clamped to it first, the sets follow
    if not general:
        boxes_b, box_b, L_b, U_b, _ = _sandwich(scene, cam, ts, row_range=(3, 5))
        rows = np.arange(box.shape[1])[None, :, None]
        assert (box_b == (box & (rows >= 3) & (rows < 5))).all()
        assert (L_b == (L & box_b)).all() and (U_b == (U & box_b)).all()


@pytest.mark.parametrize("ts", nc.TILE_SIZES)
def test_edge_boxes_have_exactly_64_65_1_and_2_tiles(ts):
    scene, meta, cam = nc.edge_scene(ts)
    boxes, box, L, U, rad = _sandwich(scene, cam, ts)
    assert tuple(box.reshape(len(box), -1).sum(1)) == nc.EDGE_BOXES
    assert tuple(boxes[0]) == (0, 8, 2, 10) and tuple(boxes[1]) == (2, 7, 0, 13)
    assert not (L & ~U).any() and L.reshape(len(L), -1).any(1).all()
    assert U[0].sum() < 0.7 * 64 and L[3].sum() == 2


def test_rect_min_against_brute_force():
    """tile_sandwich's clamped face minima equal a dense search over the rectangle."""
    rng = np.random.default_rng(3)
    for _ in range(200):
        s1, s2, th = rng.uniform(5, 60), rng.uniform(0.5, 2), rng.uniform(0, np.pi)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        Q = np.linalg.inv(R @ np.diag([s1 * s1, s2 * s2]) @ R.T)
        xl, yl = rng.uniform(-80, 60), rng.uniform(-80, 60)
        xh, yh = xl + 15.0, yl + 15.0
        got = float(nc._rect_min(np.float64(Q[0, 0]), np.float64(Q[0, 1]), np.float64(Q[1, 1]), np.float64(xl), np.float64(xh),
                                 np.float64(yl), np.float64(yh)))
        X, Y = np.meshgrid(np.linspace(xl, xh, 601), np.linspace(yl, yh, 601))
        dense = (0.5 * (Q[0, 0] * X * X + Q[1, 1] * Y * Y) + Q[0, 1] * X * Y).min()
        # (the search's step is 0.025 px and the curvature along a face at most 4: it overshoots by < 1e-3)
        assert got <= dense + 1e-12 and dense - got <= 1e-3, (got, dense)
