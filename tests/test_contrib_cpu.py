"""CPU: the definition of the contribution statistics (mojosplat_amd/contrib.py, backend="torch") and what is built on it:
the scalar restatement, the gradient identity and conservation against oracle/torch_oracle.rasterize in float64, the
bookkeeping of ContributionStats, select_by_contribution's rules, prune_scene with an optimiser attached, lift_mask."""
import math

import pytest
import torch

import mojosplat_amd as ms
from contrib_cases import (EXCUSED_CAP, Reference, cpu_lists, float32_definition, scalar_contributions, two_clusters,
                           weight_map, worst_error)
from helpers import raster_scene, simple_camera
from mojosplat_amd import (ContributionStats, GaussianAdam, accumulate_contributions, contributions_from_lists, lift_mask,
                           prune_scene, select_by_contribution)
from mojosplat_amd.binning import bin_gaussians_to_tiles_torch
from mojosplat_amd.contrib import FIXED_ONE, contributions_from_lists_torch
from mojosplat_amd.projection import project_gaussians_torch
from oracle import torch_oracle

STEP = 1.0 / FIXED_ONE


def _small_lists(dtype=torch.float64, H=20, W=24, n=30, ts=16):
    m, s, q, o, _ = raster_scene(n, seed=7, scale_log=-1.6)
    m[:, :2] *= 0.35                                       # most of the thirty land on the 24x20 image
    cam = simple_camera(H=H, W=W, f=60.0)
    m2, con, d, r = project_gaussians_torch(m, s, q, o, cam)
    ids, ranges = bin_gaussians_to_tiles_torch(m2, r, d, ts, -(-W // ts), -(-H // ts))
    return m2.to(dtype), con.to(dtype), o.to(dtype), ranges, ids, cam


@pytest.mark.parametrize("weights", [None, "random", "wild"])
def test_definition_matches_scalar_restatement(weights):
    m2, con, o, ranges, ids, cam = _small_lists()
    wmap = None if weights is None else weight_map(weights, cam.H, cam.W)
    ref = Reference(m2, con, o, ranges, ids, cam, 16, weights=wmap, keep_blended=True)
    pixels, maxw, sum_q, wsum_q, blended = scalar_contributions(m2, con, o, ranges, ids, cam.H, cam.W, 16, wmap)
    st = ref.stats
    assert sum(pixels) > 500 and sum(p > 0 for p in pixels) >= 10, "the scene must put Gaussians on the image"
    assert st.pixels.tolist() == pixels
    assert ref.blended == blended
    f32 = torch.tensor(maxw, dtype=torch.float64).float()           # max_weight is a float32 buffer
    torch.testing.assert_close(st.max_weight.double(), f32.double(), rtol=1e-12, atol=0.0)
    torch.testing.assert_close(st.weight_sum(), torch.tensor(sum_q, dtype=torch.float64) * STEP, rtol=1e-12, atol=0.0)
    torch.testing.assert_close(st.weighted_sum(), torch.tensor(wsum_q, dtype=torch.float64) * STEP, rtol=1e-12, atol=0.0)
    if weights is None:
        assert not st.wsum_q.any()


def _oracle_grad(m2, con, o, ranges, ids, cam, ts, wmap):
    colour = torch.ones(m2.shape[0], 1, dtype=torch.float64, requires_grad=True)
    img, alphas = torch_oracle.rasterize(m2, con, colour, o, None, ranges, ids, cam.H, cam.W, ts)
    (wmap.double() * img[..., 0]).sum().backward()
    return colour.grad[:, 0], alphas.detach()


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_gradient_identity_and_conservation(case):
    m2, con, o, ranges, ids, cam, ts = cpu_lists(case)
    m2, con, o = m2.double(), con.double(), o.double()
    wmap = weight_map("random", cam.H, cam.W)
    st = contributions_from_lists_torch(ContributionStats(m2.shape[0]), m2, con, o, ranges, ids, cam, weights=wmap, tile_size=ts)
    partials = torch.bincount(ids.long(), minlength=m2.shape[0]).double()     # one per tile that lists the Gaussian
    g_w, alphas = _oracle_grad(m2, con, o, ranges, ids, cam, ts, wmap)
    g_1, _ = _oracle_grad(m2, con, o, ranges, ids, cam, ts, torch.ones(cam.H, cam.W))
    for got, want in ((st.weighted_sum(), g_w), (st.weight_sum(), g_1)):
        assert bool(((got - want).abs() <= 1e-9 * want.abs() + STEP * partials).all()), (got - want).abs().max()
    total, want = float(st.weight_sum().sum()), float(alphas.sum())
    assert abs(total - want) <= 1e-9 * want + STEP * float(partials.sum())


def test_case_observations():
    """What the cases are there to exercise, on the torch stages' lists: list lengths, stopped pixels, never-blended rows; the
    near-threshold pairs stay under the cap; the float32 definition agrees with the float64 one to rounding."""
    seen = {}
    for case in ("A", "B", "C"):
        m2, con, o, ranges, ids, cam, ts = cpu_lists(case)
        ref = Reference(m2, con, o, ranges, ids, cam, ts)
        img, alphas = torch_oracle.rasterize(m2.double(), con.double(), torch.ones(len(o), 1, dtype=torch.float64), o.double(),
                                             None, ranges, ids, cam.H, cam.W, ts)
        longest = int((ranges[..., 1] - ranges[..., 0]).max())
        seen[case] = (longest, int((ref.stats.pixels > 0).sum()))
        assert int(ref.excused.sum()) <= EXCUSED_CAP * len(o)
        e32 = worst_error(float32_definition(m2, con, o, ranges, ids, cam, ts), ref, False)
        assert e32 < 5e-6, (case, e32)
        never = ref.stats.pixels == 0
        assert not ref.stats.max_weight[never].any() and not ref.stats.sum_q[never].any()
    assert seen["A"][0] > 64 and seen["B"][0] > 128 and seen["C"][0] > 256
    assert seen["C"][1] < 300, "most of case C's Gaussians are hidden"


def test_needle_case_is_what_it_says():
    """Case G on the torch stages' lists: the needles' a c and b^2 agree to better than three digits, every needle is blended in
    over a hundred pixels, and under the band that float32 can resolve the marked Gaussians stay within the cap."""
    m2, con, o, ranges, ids, cam, ts = cpu_lists("G")
    c = con[:24].double()
    assert float(((c[:, 0] * c[:, 2] - c[:, 1] ** 2) / (c[:, 0] * c[:, 2])).max()) < 1e-3
    ref = Reference(m2, con, o, ranges, ids, cam, ts, float32_sigma_band=True)
    assert bool((ref.stats.pixels[:24] > 100).all())
    assert int(ref.excused.sum()) <= EXCUSED_CAP * len(o)
    f32 = float32_definition(m2, con, o, ranges, ids, cam, ts)
    ok = ~ref.excused
    assert torch.equal(f32.pixels[ok], ref.stats.pixels[ok])


def test_two_views_add_and_weights_none_leaves_wsum():
    m2, con, o, ranges, ids, cam, ts = cpu_lists("A")
    wmap = weight_map("random", cam.H, cam.W)
    one = contributions_from_lists(ContributionStats(len(o)), m2, con, o, ranges, ids, cam, weights=wmap, backend="torch")
    m2b = m2 + torch.tensor([3.25, -1.5])
    other = contributions_from_lists(ContributionStats(len(o)), m2b, con, o, ranges, ids, cam, weights=wmap, backend="torch")
    both = ContributionStats(len(o))
    both.wsum_q += 7
    contributions_from_lists(both, m2, con, o, ranges, ids, cam, backend="torch")          # no map: wsum_q untouched
    assert bool((both.wsum_q == 7).all()) and torch.equal(both.sum_q, one.sum_q)
    both.wsum_q -= 7
    both.reset()
    contributions_from_lists(both, m2, con, o, ranges, ids, cam, weights=wmap, backend="torch")
    contributions_from_lists(both, m2b, con, o, ranges, ids, cam, weights=wmap, backend="torch")
    assert torch.equal(both.pixels, one.pixels + other.pixels)
    assert torch.equal(both.sum_q, one.sum_q + other.sum_q) and torch.equal(both.wsum_q, one.wsum_q + other.wsum_q)
    assert torch.equal(both.max_weight, torch.maximum(one.max_weight, other.max_weight))
    assert float(one.weighted_sum().sum()) < float(one.weight_sum().sum())


def test_wild_weights_equal_their_clamped_twin():
    m2, con, o, ranges, ids, cam, ts = cpu_lists("B")
    a = contributions_from_lists(ContributionStats(len(o)), m2, con, o, ranges, ids, cam, backend="torch",
                                 weights=weight_map("wild", cam.H, cam.W))
    b = contributions_from_lists(ContributionStats(len(o)), m2, con, o, ranges, ids, cam, backend="torch",
                                 weights=weight_map("wild_clamped", cam.H, cam.W))
    assert torch.equal(a.wsum_q, b.wsum_q) and a.wsum_q.any()


def test_accumulate_is_project_bin_and_lists():
    (m, s, q, o, _), cam = raster_scene(200, seed=3), simple_camera(H=64, W=64, f=60.0)
    st = accumulate_contributions(ContributionStats(200), m, s, q, o, cam, backend="torch")
    m2, con, o2, ranges, ids, cam2, ts = cpu_lists("A")
    want = contributions_from_lists(ContributionStats(200), m2, con, o2, ranges, ids, cam2, backend="torch")
    for name in ("pixels", "max_weight", "sum_q", "wsum_q"):
        assert torch.equal(getattr(st, name), getattr(want, name)), name


def test_stats_bookkeeping():
    st = ContributionStats(5)
    assert st.n == 5 and st.device.type == "cpu"
    assert (st.pixels.dtype, st.max_weight.dtype, st.sum_q.dtype, st.wsum_q.dtype) == \
        (torch.int64, torch.float32, torch.int64, torch.int64)
    st.pixels += torch.arange(5)
    st.max_weight += torch.arange(5) * 0.1
    st.sum_q += torch.arange(5) * FIXED_ONE
    st.wsum_q += torch.arange(5) * (FIXED_ONE // 2)
    assert st.weight_sum().dtype == torch.float64 and st.weight_sum().tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert st.weighted_sum().tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]
    kept = st.select(torch.tensor([True, False, True, False, True]))
    assert kept.n == 3 and kept.pixels.tolist() == [0, 2, 4] and kept.sum_q.tolist() == [0, 2 * FIXED_ONE, 4 * FIXED_ONE]
    gathered = st.select(torch.tensor([4, 4, 1]))
    assert gathered.pixels.tolist() == [4, 4, 1] and gathered.max_weight.is_contiguous()
    assert kept.append(2) is kept and kept.n == 5 and kept.pixels.tolist() == [0, 2, 4, 0, 0]
    assert kept.wsum_q.dtype == torch.int64 and kept.max_weight.dtype == torch.float32
    kept.check(5, torch.device("cpu"))
    assert kept.reset() is kept and not kept.pixels.any() and not kept.max_weight.any() and not kept.sum_q.any()
    with pytest.raises(ValueError, match=r"shape \[6\]"):
        kept.check(6, torch.device("cpu"))
    kept.sum_q = kept.sum_q.float()
    with pytest.raises(ValueError, match="int64"):
        kept.check(5, torch.device("cpu"))
    strided = ContributionStats(4)
    strided.pixels = torch.zeros(8, dtype=torch.int64)[::2]
    with pytest.raises(ValueError, match="contiguous"):
        strided.check(4, torch.device("cpu"))


def _stats(pixels, sum_q, max_weight):
    st = ContributionStats(len(pixels))
    st.pixels += torch.tensor(pixels)
    st.sum_q += torch.tensor(sum_q)
    st.max_weight += torch.tensor(max_weight)
    return st


def test_select_by_contribution_rules():
    #            row:   0    1    2    3    4    5    6
    st = _stats(pixels=[3, 1, 0, 2, 5, 0, 1], sum_q=[50, 90, 0, 50, 90, 70, 10], max_weight=[.5, .02, 0., .005, .3, .9, .01])
    # by sum_q: rows 1 and 4 tie (the lower row first), then 0 and 3 tie, then 6; 2 and 5 were never blended: last, by row
    order = [1, 4, 0, 3, 6, 2, 5]
    for f, k in ((0.0, 0), (0.1, 1), (1 / 7, 1), (0.15, 2), (0.3, 3), (0.5, 4), (5 / 7, 5), (0.75, 6), (1.0, 7)):
        keep = select_by_contribution(st, keep_fraction=f)
        assert keep.dtype == torch.bool and sorted(torch.nonzero(keep).flatten().tolist()) == sorted(order[:k]), (f, k)
    assert k == math.ceil(1.0 * 7)
    assert select_by_contribution(st, min_max_weight=0.01).tolist() == [True, True, False, False, True, True, True]
    both = select_by_contribution(st, min_max_weight=0.01, keep_fraction=0.5)           # {1, 4, 0, 3} and the rule above
    assert both.tolist() == [True, True, False, False, True, False, False]
    ten = _stats(pixels=[1] * 10, sum_q=list(range(10, 0, -1)), max_weight=[0.1] * 10)
    assert int(select_by_contribution(ten, keep_fraction=0.3).sum()) == 3                 # ceil(0.3 * 10) is 3, not 4
    assert int(select_by_contribution(ten, keep_fraction=0.3 + 1e-12).sum()) == 4         # ... and this one is above 3
    with pytest.raises(ValueError):
        select_by_contribution(st)
    with pytest.raises(ValueError, match="keep_fraction"):
        select_by_contribution(st, keep_fraction=1.5)
    with pytest.raises(ValueError, match="min_max_weight"):
        select_by_contribution(st, min_max_weight=-1.0)


def test_prune_scene_with_optimiser():
    g = torch.Generator().manual_seed(2)
    N = 9
    params = {"means3d": torch.randn(N, 3, generator=g).requires_grad_(True), "opacities": torch.randn(N, generator=g).requires_grad_(True),
              "features": torch.randn(N, 4, 3, generator=g).requires_grad_(True)}
    opt = GaussianAdam(params, lr=1e-2, backend="torch")
    for _ in range(3):
        for p in params.values():
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    moments = {n: (opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for n, p in params.items()}
    keep = torch.tensor([True, False, True, True, False, False, True, False, True])
    new = prune_scene(params, keep, opt, requires_grad=True)
    assert list(new) == list(params)
    for n, p in new.items():
        assert p.is_leaf and p.requires_grad and p.is_contiguous() and torch.equal(p.detach(), params[n].detach()[keep])
        st = opt.state[p]
        assert int(st["step"]) == 3
        assert torch.equal(st["exp_avg"], moments[n][0][keep]) and torch.equal(st["exp_avg_sq"], moments[n][1][keep])
        assert opt.group(n)["params"][0] is p
    plain = prune_scene(params, keep)
    assert all(not p.requires_grad and p.shape[0] == 5 for p in plain.values())
    with pytest.raises(ValueError, match="boolean"):
        prune_scene(params, torch.arange(3))
    with pytest.raises(ValueError, match="rows"):
        prune_scene(params, keep[:-1])


def test_lift_mask_selects_one_cluster():
    m, s, q, o = two_clusters(12)
    cam = simple_camera(H=64, W=64, f=60.0)
    mask = torch.zeros(64, 64, dtype=torch.bool)
    mask[:, :32] = True
    selected, ratio = lift_mask(m, s, q, o, cam, mask, backend="torch")
    assert selected.dtype == torch.bool and ratio.dtype == torch.float64
    assert selected.tolist() == [True] * 12 + [False] * 12
    assert bool((ratio[:12] > 0.99).all()) and bool((ratio[12:] < 0.01).all())
    # two views (the second shifted, with the mask moved along), and a threshold nothing passes
    cam2 = simple_camera(H=64, W=64, f=60.0, T=(0.2, 0.0, 0.0))
    mask2 = torch.zeros(64, 64, dtype=torch.bool)
    mask2[:, :36] = True
    selected2, _ = lift_mask(m, s, q, o, [cam, cam2], [mask, mask2], backend="torch")
    assert torch.equal(selected2, selected)
    assert not lift_mask(m, s, q, o, cam, mask, threshold=1.0, backend="torch")[0].any()
    with pytest.raises(ValueError, match="equally long"):
        lift_mask(m, s, q, o, [cam, cam2], [mask], backend="torch")


def test_argument_errors_come_before_any_work():
    m2, con, o, ranges, ids, cam, ts = cpu_lists("A")
    st = ContributionStats(len(o))
    args = (m2, con, o, ranges, ids, cam)
    with pytest.raises(ValueError, match="tile_size"):
        contributions_from_lists(st, *args, tile_size=8, backend="torch")
    with pytest.raises(ValueError, match="Invalid backend"):
        contributions_from_lists(st, *args, backend="cuda")
    with pytest.raises(ValueError, match=r"\(200, 3\)"):
        contributions_from_lists(st, m2, con[:, :2], o, ranges, ids, cam, backend="torch")
    with pytest.raises(ValueError, match=r"tile_ranges.*\(4, 4, 2\)"):
        contributions_from_lists(st, m2, con, o, ranges[:3], ids, cam, backend="torch")
    with pytest.raises(ValueError, match="sorted_ids"):
        contributions_from_lists(st, m2, con, o, ranges, ids.float(), cam, backend="torch")
    with pytest.raises(ValueError, match=r"weights.*\(64, 64\)"):
        contributions_from_lists(st, *args, weights=torch.zeros(64, 63), backend="torch")
    with pytest.raises(ValueError, match=r"stats\.pixels.*\[200\]"):
        contributions_from_lists(ContributionStats(199), *args, backend="torch")
    with pytest.raises(ValueError, match="camera must be a Camera"):
        contributions_from_lists(st, m2, con, o, ranges, ids, (64, 64), backend="torch")
    scene = raster_scene(200, seed=3)[:4]
    with pytest.raises(ValueError, match="camera must be a Camera"):
        accumulate_contributions(st, *scene, None, backend="torch")
    with pytest.raises(ValueError, match="positive integers"):
        lift_mask(*scene, simple_camera(H=0, W=64), torch.zeros(0, 64), backend="torch")
    with pytest.raises((ValueError, ms._hip.HipBackendError)):                         # CPU tensors: no fallback behind "hip"
        contributions_from_lists(st, *args, backend="hip")
    assert not st.pixels.any() and not st.sum_q.any()


def test_abi_declares_and_exports_the_entry():
    from mojosplat_amd import _hip
    lib = _hip.load()
    assert hasattr(lib, "ms_contrib_accumulate") and "ms_contrib_accumulate" in _hip.EXPORTS
    import ctypes
    P, n = ctypes.c_void_p(0x1000), ctypes.c_int64(10)
    INVALID, TOO_LARGE = 1, 3
    call = lib.ms_contrib_accumulate
    assert call(ctypes.c_int64(-1), n, P, P, P, P, P, None, 8, 8, 16, P, P, P, None, None) == INVALID
    assert call(n, n, P, P, P, P, P, None, 8, 8, 24, P, P, P, None, None) == INVALID
    assert b"tile_size" in lib.ms_last_error_string()
    assert call(n, n, P, P, P, P, P, None, 0, 8, 16, P, P, P, None, None) == INVALID
    assert call(n, n, None, P, P, P, P, None, 8, 8, 16, P, P, P, None, None) == INVALID
    assert call(n, n, P, P, P, P, P, P, 8, 8, 16, P, P, P, None, None) == INVALID          # weights without wsum_q
    assert call(n, n, P, P, P, P, P, None, 8, 8, 16, ctypes.c_void_p(0x1004), P, P, None, None) == INVALID
    assert call(ctypes.c_int64(2 ** 31), n, P, P, P, P, P, None, 8, 8, 16, P, P, P, None, None) == TOO_LARGE
    assert call(ctypes.c_int64(0), n, None, None, None, None, None, None, 8, 8, 16, None, None, None, None, None) == 0
