"""Needle and edge-on disc Gaussians for tests/test_needles_cpu.py and tests/test_hip_needles.py: the generators and the
float64 references the drop decisions are held to ("Needles").

Two pieces of code decide which Gaussians a pixel ever sees -- reach_mask (csrc/binning.hip, tight binning) and the quad
reach test (csrc/rasterize.hip, fed by ms_common.hpp's make_raster_record).  Both form det = ca cc - cb^2 and a clamped
1-D minimum in float32, which cancel on exactly the footprints they exist for.  Nothing here is held to a pixel bar: the
references bound the DISCRETE decisions (tile_sandwich: a lower and an upper set of (Gaussian, tile) pairs) and the one
exponent every pixel evaluates (alpha_reference + rule_p)."""
import math

import numpy as np
import torch

from helpers import camera_by_name, simple_camera

FIXED_DEG = (0.0, 45.0, 90.0, 135.0, 1.0, -1.0, 89.0, 91.0, 44.0, 46.0, 134.0, 136.0)
ASPECTS = (10.0, 100.0, 1000.0)
# 0.002: culled (< 1/255 = 0.00392); 0.004 and 1/255 + 1e-4: just above it, a footprint of a few pixels; 0.9995 and 1.0: the
# 0.999 clamp can bind, the record reports "no bound" and the rasteriser takes its generic loop
OPACITIES = (0.002, 0.004, 1.0 / 255.0 + 1e-4, 0.05, 0.5, 0.99, 0.9995, 1.0)
TILE_SIZES = (8, 16, 32, 64)
NEEDLE, DISC, BORDER = 0, 1, 2
N_NEEDLES, N_DISCS, N_BORDER = 24, 9, 8      # 24 = 3 * 8: every (aspect, opacity) combination once
N_SINGLE = 24                                # single-Gaussian frames per frame size: 16 needles + 8 discs
LOG2_THR = math.log2(1.0 / 255.0)
GENERAL_CAMERA = "fx>fy_pp_xy"


# ------------------------------------------------------------------ generators
def _quat_of(R):
    """Rotation matrix (3, 3) float64 -> unit quaternion wxyz (Shepperd's branches)."""
    t = np.trace(R)
    if t > 0:
        s = 2.0 * math.sqrt(1.0 + t)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q = np.asarray(q)
    return q / np.linalg.norm(q)


def _rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


class _Builder:
    """Gaussians placed in CAMERA space by what they should project to, then mapped to world (helpers.general_scene)."""

    def __init__(self, cam):
        self.cam = cam
        self.R = cam.R.detach().cpu().double().numpy()
        self.t = cam.T.detach().cpu().double().numpy()
        self.rows = []

    def add(self, u, v, z, theta_deg, sigma_px, aspect, opacity, family, tilt_deg=None):
        """Mean at pixel (u, v), depth z; major axis at in-image angle theta with a projected sigma of sigma_px.
        tilt_deg None: a needle (s, s/A, s/A) lying in the image plane; else a disc (s, s, s/A) tilted that far about
        its major axis -- seen edge-on."""
        cam = self.cam
        th = math.radians(theta_deg)
        # the in-plane 3-D direction that projects onto angle theta, and the length whose image is sigma_px
        dx, dy = math.cos(th) / cam.fx, math.sin(th) / cam.fy
        s = sigma_px * z * math.hypot(dx, dy)
        Rl = _rot_z(math.atan2(dy, dx))
        if tilt_deg is None:
            scales = (s, s / aspect, s / aspect)
        else:
            Rl = Rl @ _rot_x(math.radians(tilt_deg))
            scales = (s, s, s / aspect)
        pc = np.array([(u - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z, z])
        Rw = self.R.T @ Rl
        if np.linalg.det(Rw) < 0:          # a view matrix that mirrors (utils.look_at's is left-handed): flip one local
            Rw[:, 2] = -Rw[:, 2]           # axis -- R diag(s^2) R^T does not change, and the result is a rotation
        self.rows.append(dict(mean=self.R.T @ (pc - self.t), scales=scales, quat=_quat_of(Rw), opacity=opacity,
                              family=family, theta=theta_deg, aspect=aspect, sigma_px=sigma_px))

    def scene(self, scales_log=True, channels=3, seed=0):
        """-> dict(means3d, scales, quats, opacities, features) float32 CPU and meta dict of numpy arrays."""
        r = self.rows
        sc = torch.tensor(np.array([x["scales"] for x in r]), dtype=torch.float64)
        g = torch.Generator().manual_seed(seed)
        scene = dict(means3d=torch.tensor(np.array([x["mean"] for x in r])).float().contiguous(),
                     scales=(torch.log(sc) if scales_log else sc).float().contiguous(),
                     quats=torch.tensor(np.array([x["quat"] for x in r])).float().contiguous(),
                     opacities=torch.tensor([x["opacity"] for x in r], dtype=torch.float64).float().contiguous(),
                     features=torch.rand(len(r), channels, generator=g).contiguous())
        meta = {k: np.array([x[k] for x in r]) for k in ("family", "theta", "aspect", "sigma_px", "opacity")}
        return scene, meta


def frame_camera(ts, general=False):
    """The camera of an 8 x 8-tile frame of tile size ts -- or the general one (fx != fy, off-centre principal point;
    330 x 190: 21 x 12 tiles of 16 px, neither side a multiple of the tile)."""
    if general:
        return camera_by_name(GENERAL_CAMERA)
    return simple_camera(H=8 * ts, W=8 * ts, f=8.0 * ts)


def needle_scene(ts, *, general=False, scales_log=True, seed=0):
    """N_NEEDLES needles, N_DISCS edge-on discs and N_BORDER needles across the image border, for tile size ts.
    Angles: FIXED_DEG, then seeded random ones.  Projected major sigma: 0.03 .. 0.15 of 8 tiles, log-uniform.  Means in
    the middle two tiles of the frame (of the general camera's image: the two tiles around its centre)."""
    cam = frame_camera(ts, general)
    rng = np.random.default_rng(1000 * ts + seed)
    side = 8.0 * ts
    u0, v0 = cam.W / 2.0 - ts, cam.H / 2.0 - ts
    b = _Builder(cam)

    def angle(i):
        # (the random part stays within 25 degrees of a diagonal: the fixed list has the axes, and a needle along an axis
        # fills its box)
        return FIXED_DEG[i] if i < len(FIXED_DEG) else float(rng.choice((45.0, 135.0)) + rng.uniform(-25.0, 25.0))

    def sigma():
        return side * math.exp(rng.uniform(math.log(0.03), math.log(0.15)))

    def spot(o):
        # a faint Gaussian's footprint is a fraction of a pixel wide (o = 0.004: 0.11 px either side of the axis): its mean
        # sits on a pixel centre, so that it blends somewhere whatever its angle
        u, v = u0 + rng.uniform(0, 2 * ts), v0 + rng.uniform(0, 2 * ts)
        return (math.floor(u) + 0.5, math.floor(v) + 0.5) if o < 0.01 else (u, v)

    for i in range(N_NEEDLES):
        b.add(*spot(OPACITIES[i % 8]), rng.uniform(2.0, 6.0), angle(i), sigma(), ASPECTS[i % 3], OPACITIES[i % 8], NEEDLE)
    for i in range(N_DISCS):
        # (the opacities run backwards so that the first eight discs -- the single frames -- hold all eight)
        b.add(*spot(OPACITIES[7 - i % 8]), rng.uniform(2.0, 6.0), angle((5 * i + 1) % 15), sigma(), ASPECTS[i % 3],
              OPACITIES[7 - i % 8], DISC, tilt_deg=rng.uniform(80.0, 89.0))
    # across each border and corner: the mean a fraction of a tile outside or inside, the needle pointing inwards
    spots = [(0.0, -0.3, 0.4, 0.0, 20.0), (1.0, 0.2, 0.6, 0.0, 160.0), (0.3, 0.0, 0.0, -0.2, 70.0), (0.7, 0.0, 1.0, 0.3, 100.0),
             (0.0, -0.1, 0.0, -0.1, 45.0), (1.0, 0.1, 1.0, 0.1, 46.0), (1.0, -0.1, 0.0, 0.1, 134.0), (0.5, 0.0, 1.0, -0.01, 1.0)]
    for i, (fu, du, fv, dv, deg) in enumerate(spots[:N_BORDER]):
        b.add(fu * cam.W + du * ts, fv * cam.H + dv * ts, rng.uniform(2.0, 6.0), deg, 0.12 * side, ASPECTS[(i + 1) % 3],
              (0.5, 0.99, 0.05, 1.0)[i % 4], BORDER)
    scene, meta = b.scene(scales_log, seed=seed)
    return scene, meta, cam


SINGLE_MAX_SIGMA = 40.0


def single_cases(meta):
    """Indices of the (up to) N_SINGLE Gaussians of a needle_scene rendered alone: the first 16 needles and 8 discs whose
    projected major sigma is at most SINGLE_MAX_SIGMA px.  Why: rule_p's undecided band is e wide in the exponent and
    e grows with S, i.e. with the square of the distance along a diagonal needle (S ~ 2.4 t^2 at t px from the mean,
    minor variance 0.3), so the band's share of a frame's blending pixels grows with sigma^2: about 0.3 % at 70 px --
    6 pixels expected where the cap of 0.5 % allows 10, too close for a count that is redrawn whenever the projection's
    last bit moves -- and 0.1 % (under 2 pixels expected, 6 allowed) at 40 px.  Only frames of 64-px tiles have longer
    needles; those stay in the tile-list and scene tests."""
    ok = meta["sigma_px"] <= SINGLE_MAX_SIGMA
    n = np.flatnonzero((meta["family"] == NEEDLE) & ok)[:16]
    d = np.flatnonzero((meta["family"] == DISC) & ok)[:8]
    return [int(i) for i in np.concatenate([n, d])]


def single_scene(scene, i):
    """Gaussian i alone, colour 1."""
    sc = {k: v[i:i + 1].clone() for k, v in scene.items()}
    sc["features"] = torch.ones_like(sc["features"])
    return sc


EDGE_BOXES = (64, 65, 1, 2)


def edge_scene(ts):
    """Four Gaussians whose tile boxes have exactly EDGE_BOXES tiles -- the reach mask's on/off edges: 8 x 8 (the largest
    masked box), 5 x 13 clipped by the image (65: kept whole), 1 x 1 (kept whole) and 2 x 1 (the smallest masked box).
    Frame: 8 x 13 tiles."""
    cam = simple_camera(H=13 * ts, W=8 * ts, f=8.0 * ts)
    b = _Builder(cam)
    ext = math.sqrt(2.0 * math.log(255.0 * 0.99))             # the opacity-aware extent at o = 0.99 (< 3.33)
    # 8 x 8: a 45-degree needle with radii of 3.5 tiles, mean on a tile corner
    cxx = (3.5 * ts / ext) ** 2
    b.add(4.0 * ts, 6.0 * ts, 3.0, 45.0, math.sqrt(2.0 * (cxx - 0.3)), 30.0, 0.99, NEEDLE)
    # 5 x 13: radii 2 and 7 tiles about the centre of tile (4, 6): rows -1 .. 13 clipped to the 13 the image has
    sx, sy = (2.0 * ts / ext) ** 2 - 0.3, (7.0 * ts / ext) ** 2 - 0.3
    b.add(4.5 * ts, 6.5 * ts, 3.0, math.degrees(math.atan2(math.sqrt(sy), math.sqrt(sx))), math.sqrt(sx + sy), 100.0, 0.99,
          NEEDLE)
    # 1 x 1: a point at a tile's centre (radius 2 px); 2 x 1: the same on a vertical tile boundary
    b.add(2.5 * ts, 2.5 * ts, 3.0, 0.0, 0.1, 1.0, 0.99, NEEDLE)
    b.add(3.0 * ts, 9.5 * ts, 3.0, 0.0, 0.1, 1.0, 0.99, NEEDLE)
    scene, meta = b.scene(True)
    return scene, meta, cam


def needle_cloud(N, cam, seed=0):
    """N overlapping needles and discs all over the frame: aspects 10 .. 1000, FIXED_DEG and random angles, projected
    major sigma 3 .. 60 px, depths 2 .. 8, opacities 0.05 .. 0.99 with every 16th from OPACITIES."""
    rng = np.random.default_rng(seed)
    b = _Builder(cam)
    for i in range(N):
        deg = FIXED_DEG[i % 16] if i % 16 < len(FIXED_DEG) else float(rng.uniform(0.0, 180.0))
        o = OPACITIES[(i // 16) % 8] if i % 16 == 0 else float(rng.uniform(0.05, 0.99))
        b.add(rng.uniform(-0.05, 1.05) * cam.W, rng.uniform(-0.05, 1.05) * cam.H, rng.uniform(2.0, 8.0), deg,
              math.exp(rng.uniform(math.log(3.0), math.log(60.0))), float(10.0 ** rng.uniform(1.0, 3.0)), o,
              DISC if i % 4 == 3 else NEEDLE, tilt_deg=rng.uniform(80.0, 89.0) if i % 4 == 3 else None)
    return b.scene(True, seed=seed)[0]


# ------------------------------------------------------------------ gsplat tile boxes (float32, as tile_bbox)
def tile_boxes(means2d, radii, ts, tw, th, row_range=None):
    """-> (N, 4) int64 [x0, x1, y0, y1): the gsplat box clamped to the grid, then to the band; empty for radii <= 0."""
    m, r = np.asarray(means2d, np.float32), np.asarray(radii)
    f = np.float32(ts)
    tx, ty, rx, ry = m[:, 0] / f, m[:, 1] / f, r[:, 0].astype(np.float32) / f, r[:, 1].astype(np.float32) / f
    x0, x1 = np.clip(np.floor(tx - rx), 0, tw), np.clip(np.ceil(tx + rx), 0, tw)
    y0, y1 = np.clip(np.floor(ty - ry), 0, th), np.clip(np.ceil(ty + ry), 0, th)
    r0, r1 = (0, th) if row_range is None else row_range
    y0, y1 = np.maximum(y0, r0), np.minimum(y1, r1)
    y1 = np.maximum(y1, y0)
    box = np.stack([x0, x1, y0, y1], 1).astype(np.int64)
    box[~((r[:, 0] > 0) & (r[:, 1] > 0))] = 0
    return box


def box_pairs(boxes, tw, th):
    """(N, 4) boxes -> (N, th, tw) bool."""
    X, Y = np.arange(tw)[None, None, :], np.arange(th)[None, :, None]
    b = boxes[:, :, None, None]
    return (X >= b[:, 0]) & (X < b[:, 1]) & (Y >= b[:, 2]) & (Y < b[:, 3])


# ------------------------------------------------------------------ the references
def alpha_reference(means2d, conics, opacity, H, W):
    """The exponent every rasteriser path evaluates, for each Gaussian at each pixel centre: (N, H, W) float64 each of
      la64 = a' dx^2 + b' dx dy + c' dy^2 + log2 o,  S = |a'| dx^2 + |b'| |dx dy| + |c'| dy^2 + |log2 o|,
      e = 8 * 2^-24 * S + 2^-21.
    Inputs are the kernel's own float32 outputs.  dx = fl32(mx - px), dy likewise, and the record's a', b', c', log2 o are
    formed in float32 as make_raster_record writes them; everything else is float64.  e bounds |fp32 exponent - la64|:
    at most five roundings of intermediates bounded by S, one ulp each on a', b', c' for how the constant is associated,
    v_log / v_exp at about 2^-22 -- rounded up to 8 (a float32 numpy emulation's worst case was 3.2)."""
    m = np.asarray(means2d, np.float32).reshape(-1, 2)
    c = np.asarray(conics, np.float32).reshape(-1, 3)
    o = np.asarray(opacity, np.float32).reshape(-1)
    k = np.float32(1.4426950408889634)
    a_ = (np.float32(-0.5) * k) * c[:, 0]
    b_ = (-k) * c[:, 1]
    c_ = (np.float32(-0.5) * k) * c[:, 2]
    with np.errstate(divide="ignore"):
        l2o = np.log2(o.astype(np.float64)).astype(np.float32)
    px = (np.arange(W, dtype=np.float32) + np.float32(0.5))[None, None, :]
    py = (np.arange(H, dtype=np.float32) + np.float32(0.5))[None, :, None]
    dx = (m[:, 0, None, None] - px).astype(np.float64)      # float32 subtraction, then widened
    dy = (m[:, 1, None, None] - py).astype(np.float64)
    A, B, C, Lo = (v.astype(np.float64)[:, None, None] for v in (a_, b_, c_, l2o))
    la = A * dx * dx + B * dx * dy + C * dy * dy + Lo
    S = np.abs(A) * dx * dx + np.abs(B) * np.abs(dx * dy) + np.abs(C) * dy * dy + np.abs(Lo)
    return la, S, 8.0 * 2.0 ** -24 * S + 2.0 ** -21


def rule_p(frame, la, e, opacity):
    """Rule P for a single-Gaussian frame (colour 1, black background: the pixel IS alpha).  frame, la, e: (H, W).
      must:   la - e >= log2(1/255) + 2^-20  ->  pixel > 0 and |log2 pixel - min(la, log2 0.999 if o > 0.999)| <= e + 2^-20
      never:  la + e <  log2(1/255)          ->  pixel == 0 exactly
      in between either is allowed (and a blended pixel there still obeys the must-bound).
    -> dict(blending, undecided, share, worst): pixels with la >= the threshold, pixels in between, their ratio, the
    largest |log2 pixel - la| / (e + 2^-20) over the blended pixels; `bad`: the violations (asserted by the caller)."""
    frame = np.asarray(frame, np.float64)
    must = la - e >= LOG2_THR + 2.0 ** -20
    never = la + e < LOG2_THR
    if not (opacity >= 1.0 / 255.0):
        must, never = np.zeros_like(must), np.ones_like(never)
    target = np.minimum(la, math.log2(0.999)) if opacity > 0.999 else la
    on = frame > 0
    with np.errstate(divide="ignore"):
        err = np.where(on, np.abs(np.log2(np.where(on, frame, 1.0)) - target), 0.0)
    ratio = err / (e + 2.0 ** -20)
    bad = dict(zero_where_it_must_blend=int((must & ~on).sum()), blended_where_it_never_may=int((never & on).sum()),
               off_the_exponent=int((on & ~never & (ratio > 1.0)).sum()))
    blending = int((la >= LOG2_THR).sum()) if opacity >= 1.0 / 255.0 else 0
    undecided = int((~must & ~never).sum())
    return dict(blending=blending, undecided=undecided, share=undecided / max(blending, 1),
                worst=float(ratio[on & ~never].max()) if (on & ~never).any() else 0.0, bad=bad,
                undecided_mask=~must & ~never)


UNDECIDED_CAP = 5e-3      # of a frame's blending pixels


def _rect_min(a, b, c, xl, xh, yl, yh):
    """min over the rectangle [xl, xh] x [yl, yh] of sigma(d) = (a dx^2 + c dy^2) / 2 + b dx dy, a convex quadratic
    (float64 arrays, broadcast): 0 if the origin is inside, else the least of the four faces' clamped 1-D minima."""
    def sig(x, y):
        return 0.5 * (a * x * x + c * y * y) + b * x * y
    best = np.full(np.broadcast(a, xl, yl).shape, np.inf)
    for X in (xl, xh):
        y = np.clip(-b * X / c, yl, yh)
        best = np.minimum(best, sig(X, y))
    for Y in (yl, yh):
        x = np.clip(-b * Y / a, xl, xh)
        best = np.minimum(best, sig(x, Y))
    inside = (xl <= 0) & (xh >= 0) & (yl <= 0) & (yh >= 0)
    return np.where(inside, 0.0, best)


def tile_sandwich(means2d, conics, opacity, boxes, ts, tw, th):
    """Float64 bounds on tight binning, from the kernel's own float32 means2d / conics.  For each tile of each
    Gaussian's box (boxes: (N, 4) [x0, x1, y0, y1)), the exact minimum of sigma over the tile's pixel-centre rectangle.
      L (must be kept):  min over the exact rectangle            <= s (1 - 1e-3) - 1e-3
      U (may be kept):   min over the rectangle grown by 0.05 px <= s * 1.001 + 1e-3,        s = ln(255 o)
    The margins are the kernel's documented padding (0.01 px, 1.0001 s + 1e-4) times 5 - 10: a harmless extra pair
    from the cancelling det does not fail a test, a dropped pair the rasteriser would blend does.
    -> L, U: (N, th, tw) bool, both inside the boxes."""
    m = np.asarray(means2d, np.float64).reshape(-1, 2)
    q = np.asarray(conics, np.float64).reshape(-1, 3)
    o = np.asarray(opacity, np.float64).reshape(-1)
    inbox = box_pairs(np.asarray(boxes), tw, th)
    a, b, c = (q[:, k, None, None] for k in range(3))
    xl = (np.arange(tw) * ts + 0.5)[None, None, :] - m[:, 0, None, None]
    yl = (np.arange(th) * ts + 0.5)[None, :, None] - m[:, 1, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.log(255.0 * o)[:, None, None]
        exact = _rect_min(a, b, c, xl, xl + (ts - 1), yl, yl + (ts - 1))
        grown = _rect_min(a, b, c, xl - 0.05, xl + (ts - 1) + 0.05, yl - 0.05, yl + (ts - 1) + 0.05)
        L = inbox & (exact <= s * (1.0 - 1e-3) - 1e-3)
        U = inbox & (grown <= s * 1.001 + 1e-3)
    return L, U


def lists_to_pairs(ids, ranges, N):
    """Sorted per-tile lists -> (N, th, tw) bool."""
    th, tw = ranges.shape[:2]
    out = np.zeros((N, th, tw), bool)
    for y in range(th):
        for x in range(tw):
            a, b = ranges[y, x]
            out[ids[a:b], y, x] = True
    return out
