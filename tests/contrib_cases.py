"""Shared scenes, the scalar restatement and the float64 reference of the contribution statistics (mojosplat_amd/contrib.py).

Cases (helpers.raster_scene, simple_camera(f=60)); what each exercises:
  A  raster_scene(200, seed=3), 64x64          longest list 86 entries: more than one staging batch; no pixel stops
  B  raster_scene(400, seed=3), W=52, H=70     ragged tiles on both edges; longest list 163; some pixels stop
  C  raster_scene(600, seed=3, scale_log=-1.2, opacity_range=(0.8, 0.99)), 48x48
                                               lists up to 460, every pixel stops, most Gaussians are never blended
  D  one Gaussian over every tile of 80x48     all cross-tile accumulation goes into one row
  E  a scene wholly behind the camera          M = 0: nothing may be written
  F  case B at tile_size=32                    the second supported tile size
  G  24 needles among 176 of case A's Gaussians, 64x64
                                               long thin rotated Gaussians (major sigma 300 px, minor 0.1 px before the 0.3 px^2
                                               dilation) that cross every tile, most of them far from their means: a*c and b*b
                                               of their conics agree to four or five digits, so a reach test through the
                                               float32 determinant drops pixels that the exact rule blends

The GPU comparison (tests/test_hip_contrib.py).  The reference is the definition in float64 on the lists the HIP stages made.
It marks each (pixel, entry) pair whose 255 alpha lies within BAND of 1 while the pixel is alive, or whose T_after / 1e-4
lies within BAND of 1 (the band of the project's parity records): a float32 walk may decide such a pair the other way.  A
Gaussian with such a pair of its own is excused from the exact bars (pixels equal, max_weight == 0 exactly where the
reference's is); at most 1 % of N may be excused, a condition on the inputs.  Sums and max_weight:
|hip - ref| <= bar (|ref| + 1e-3) + slack_i, with slack_i from the reference alone -- max(w, T_before / 255) for a marked pair
of Gaussian i, w / 255 + 1e-4 for every entry of i behind a marked pair in its pixel -- and bar = 8 x the worst error of the
float32 torch definition against the float64 one under the same formula (8: the kernel's other exp and order of operations),
computed per case in the test, never from HIP output.

Case G alone widens the band per pair by what float32 can resolve there.  A float32 evaluation of sigma carries up to
4 * 2^-24 * S, S = 0.5 (|a| dx^2 + |c| dy^2) + |b dx dy| the sum of the magnitudes of its terms (six roundings, each at most
2^-24 of a partial sum that S bounds; the subtraction mean - pixel adds less).  Along a needle S grows to 1.5 r^2 at r pixels
from the mean (1.2e4 at 90 px: 3e-3 in sigma, against 2e-5), so a pair within 2e-5 + 4 * 2^-24 * S of the alpha threshold is
marked, and for the stop rule the same widths accumulate over the entries blended before, d log T = -alpha dsigma / (1 - alpha).
On cases A-F (S of a few tens) this would add 1e-5 at most and is not applied.  The cap of 1 % stays.

Measured on an MI355X (worst (|hip - ref| - slack) / (|ref| + 1e-3) over sum, weighted sum and max_weight, beside the bar):
  A 5.0e-7 (bar 2.5e-6)   B 5.9e-7 (3.7e-6), the same under the three weight maps   C 6.4e-7 (4.9e-6; one marked pair,
  one Gaussian excused, slack 0.02 of a total weight of 2303)   D 1.5e-8 (4.2e-8)   F 5.9e-7 (3.7e-6)
  G 2.7e-4 (2.2e-3; one marked pair, one Gaussian excused, slack 0.0072 of a total weight of 3139)
"""
import functools
import math

import torch

from helpers import raster_scene, simple_camera
from mojosplat_amd import ContributionStats
from mojosplat_amd.contrib import FIXED_ONE, contributions_from_lists_torch

BAND = 2e-5
EXCUSED_CAP = 0.01


# ------------------------------------------------------------------------------------------------------------------ scenes
def case_scene(name):
    """-> (means3d, log scales, quats, opacities) float32 CPU tensors, (H, W), tile_size."""
    if name in ("A", "B", "C", "F"):
        n, kw, hw = {"A": (200, {}, (64, 64)), "B": (400, {}, (70, 52)), "F": (400, {}, (70, 52)),
                     "C": (600, dict(scale_log=-1.2, opacity_range=(0.8, 0.99)), (48, 48))}[name]
        m, s, q, o, _ = raster_scene(n, seed=3, **kw)
        return (m, s, q, o), hw, 32 if name == "F" else 16
    if name == "G":
        g = torch.Generator().manual_seed(21)
        m, s, q, o, _ = raster_scene(176, seed=3)
        k = 24
        mn = torch.stack([(torch.rand(k, generator=g) - 0.5) * 2.8, (torch.rand(k, generator=g) - 0.5) * 2.8,
                          torch.full((k,), 3.0)], 1)                       # projected inside the 64x64 image
        sn = torch.log(torch.tensor([15.0, 0.005, 0.005])).repeat(k, 1)  # 60 * 15 / 3 = 300 px along the major axis
        th = torch.rand(k, generator=g) * math.pi                          # rotated in the image plane
        qn = torch.stack([torch.cos(th / 2), torch.zeros(k), torch.zeros(k), torch.sin(th / 2)], 1)
        on = torch.rand(k, generator=g) * 0.45 + 0.5
        return (torch.cat([mn, m]), torch.cat([sn, s]), torch.cat([qn, q]), torch.cat([on, o])), (64, 64), 16
    if name == "D":     # sigma = f s / z = 60 px on an 80x48 image: alpha >= 0.9 exp(-0.5 (47 / 60)^2) everywhere
        return (torch.tensor([[0.0, 0.0, 2.0]]), torch.full((1, 3), math.log(2.0)), torch.tensor([[1.0, 0.0, 0.0, 0.0]]),
                torch.tensor([0.9])), (48, 80), 16
    if name == "E":
        m, s, q, o, _ = raster_scene(50, seed=3)
        m[:, 2] = -m[:, 2]
        return (m, s, q, o), (64, 64), 16
    raise KeyError(name)


def case_camera(name, device="cpu", T=(0.0, 0.0, 0.0)):
    _, (H, W), _ = case_scene(name)
    return simple_camera(device=device, H=H, W=W, f=60.0, T=T)


def weight_map(kind, H, W):
    """'random': uniform in [0, 1]; 'binary': a mask; 'wild': values outside [0, 1] and a NaN; 'wild_clamped': its twin."""
    g = torch.Generator().manual_seed(11)
    if kind == "random":
        return torch.rand(H, W, generator=g)
    if kind == "binary":
        return (torch.rand(H, W, generator=g) < 0.4).float()
    w = torch.rand(H, W, generator=g) * 3.0 - 1.0
    w[H // 2, W // 3] = float("nan")
    w[1, 1], w[2, 2] = float("inf"), float("-inf")
    if kind == "wild":
        return w
    if kind == "wild_clamped":
        return torch.nan_to_num(w, nan=0.0, posinf=1.0, neginf=0.0).clamp(0.0, 1.0)
    raise KeyError(kind)


def two_clusters(n=12):
    """Two separated clusters (rows [0, n) left of the image's middle, rows [n, 2 n) right of it) for a 64x64 f=60 camera."""
    g = torch.Generator().manual_seed(5)
    m = (torch.rand(2 * n, 3, generator=g) - 0.5) * 0.8
    m[:, 2] = 3.0 + m[:, 2] * 0.5
    m[:n, 0] -= 1.0
    m[n:, 0] += 1.0
    s = torch.full((2 * n, 3), -3.0)
    q = torch.nn.functional.normalize(torch.randn(2 * n, 4, generator=g), dim=1)
    o = torch.rand(2 * n, generator=g) * 0.3 + 0.3
    return m, s, q, o


# ------------------------------------------------------------------------------------------- the scalar restatement
def scalar_contributions(means2d, conics, opacities, tile_ranges, ids, H, W, ts, weights=None):
    """The rules of the issue, one pixel and one entry at a time, in Python floats (float64).
    -> pixels [N] ints, max_weight [N] floats, sum_q [N] ints, wsum_q [N] ints, the set of blended (y, x, Gaussian)."""
    m, c, o = means2d.tolist(), conics.tolist(), opacities.reshape(-1).tolist()
    ranges, ids = tile_ranges.tolist(), ids.tolist()
    N = len(m)
    pixels, maxw, sum_q, wsum_q, blended = [0] * N, [0.0] * N, [0] * N, [0] * N, set()
    wt = None
    if weights is not None:
        wt = [[0.0 if v != v else min(max(v, 0.0), 1.0) for v in row] for row in weights.tolist()]
    for ty in range(len(ranges)):
        for tx in range(len(ranges[0])):
            s, e = ranges[ty][tx]
            part, wpart = {}, {}
            for y in range(ty * ts, min(ty * ts + ts, H)):
                for x in range(tx * ts, min(tx * ts + ts, W)):
                    T, px, py = 1.0, x + 0.5, y + 0.5
                    for k in range(s, e):
                        g = ids[k]
                        dx, dy = m[g][0] - px, m[g][1] - py
                        sigma = 0.5 * (c[g][0] * dx * dx + c[g][2] * dy * dy) + c[g][1] * dx * dy
                        if sigma < 0:
                            continue
                        alpha = min(0.999, o[g] * math.exp(-sigma))
                        if alpha < 1.0 / 255.0:
                            continue
                        after = T * (1.0 - alpha)
                        if after <= 1e-4:
                            break
                        w = alpha * T
                        T = after
                        pixels[g] += 1
                        maxw[g] = max(maxw[g], w)
                        part[g] = part.get(g, 0.0) + w
                        if wt is not None:
                            wpart[g] = wpart.get(g, 0.0) + w * wt[y][x]
                        blended.add((y, x, g))
            for g, p in part.items():
                sum_q[g] += round(p * FIXED_ONE)          # (round(): to nearest, ties to even, as llrint)
            for g, p in wpart.items():
                wsum_q[g] += round(p * FIXED_ONE)
    return pixels, maxw, sum_q, wsum_q, blended


# ------------------------------------------------------------------------------------------------- the float64 reference
class Reference:
    """The float64 definition on given lists, with the marks of the module docstring: stats (ContributionStats), excused
    (bool [N]), slack (float64 [N]), blended (set of (y, x, Gaussian)) when asked for."""

    def __init__(self, means2d, conics, opacities, tile_ranges, ids, cam, tile_size, weights=None, keep_blended=False,
                 float32_sigma_band=False):
        N = means2d.shape[0]
        m64, c64 = means2d.double(), conics.double().abs()
        self.excused = torch.zeros(N, dtype=torch.bool)
        self.slack = torch.zeros(N, dtype=torch.float64)
        self.near_pairs = 0
        self.blended = set() if keep_blended else None
        W = cam.W

        def probe(ty, tx, g, xs, ys, alpha, valid, live, t_before, t_after):
            if self.blended is not None:
                k, p = torch.nonzero(live, as_tuple=True)
                self.blended.update(zip((ys[p] - 0.5).long().tolist(), (xs[p] - 0.5).long().tolist(), g[k].tolist()))
            stopped = valid & ~live                                        # the entry a pixel stops at, and valid ones behind it
            alive = (torch.cumsum(stopped, 0) - stopped.long()) == 0       # no stop before this entry
            tested = t_before * (1 - alpha)                                # what the stop rule looks at
            band_a = band_t = BAND
            if float32_sigma_band:                                         # (module docstring: what float32 resolves at this pair)
                dx, dy = (m64[g, 0][:, None] - xs[None, :]).abs(), (m64[g, 1][:, None] - ys[None, :]).abs()
                dsig = 4.0 * 2.0 ** -24 * (0.5 * (c64[g, 0][:, None] * dx * dx + c64[g, 2][:, None] * dy * dy)
                                           + c64[g, 1][:, None] * dx * dy)
                band_a = BAND + dsig
                band_t = BAND + torch.cumsum(torch.where(valid, alpha * dsig / (1 - alpha), torch.zeros_like(dsig)), 0)
            near = alive & ((255.0 * alpha - 1.0).abs() <= band_a)
            near |= alive & valid & ((tested / 1e-4 - 1.0).abs() <= band_t)
            if not bool(near.any()):
                return
            self.near_pairs += int(near.sum())
            w = alpha * t_before
            rows = g[:, None].expand_as(alpha)
            self.excused[rows[near]] = True
            self.slack.index_add_(0, rows[near], torch.maximum(w, t_before / 255.0)[near])
            behind = ((torch.cumsum(near, 0) - near.long()) > 0) & valid   # entries behind a marked pair in their pixel
            self.slack.index_add_(0, rows[behind], (w / 255.0 + 1e-4)[behind])

        self.stats = contributions_from_lists_torch(
            ContributionStats(N), means2d.double(), conics.double(), opacities.double(), tile_ranges, ids, cam,
            weights=weights, tile_size=tile_size, _probe=probe)


def rel_error(got, ref, slack):
    """max over i of (|got_i - ref_i| - slack_i) / (|ref_i| + 1e-3), float64 tensors -> float (never below 0)."""
    e = ((got.double() - ref.double()).abs() - slack) / (ref.double().abs() + 1e-3)
    return max(0.0, float(e.max())) if e.numel() else 0.0


def worst_error(stats, ref, with_weights):
    """The formula of the bound over sum, weighted sum and max_weight."""
    e = max(rel_error(stats.weight_sum(), ref.stats.weight_sum(), ref.slack),
            rel_error(stats.max_weight, ref.stats.max_weight, ref.slack))
    if with_weights:
        e = max(e, rel_error(stats.weighted_sum(), ref.stats.weighted_sum(), ref.slack))
    return e


def float32_definition(means2d, conics, opacities, tile_ranges, ids, cam, tile_size, weights=None):
    return contributions_from_lists_torch(ContributionStats(means2d.shape[0]), means2d.float(), conics.float(),
                                          opacities.float(), tile_ranges, ids, cam, weights=weights, tile_size=tile_size)


@functools.lru_cache(maxsize=None)
def cpu_lists(name):
    """The case's lists from the torch stages -> (means2d, conics, opacities, tile_ranges, ids, camera, tile_size), shared."""
    from mojosplat_amd.binning import bin_gaussians_to_tiles_torch
    from mojosplat_amd.projection import project_gaussians_torch
    (m, s, q, o), (H, W), ts = case_scene(name)
    cam = case_camera(name)
    m2, con, d, r = project_gaussians_torch(m, s, q, o, cam)
    ids, ranges = bin_gaussians_to_tiles_torch(m2, r, d, ts, -(-W // ts), -(-H // ts))
    return m2, con, o, ranges, ids, cam, ts
