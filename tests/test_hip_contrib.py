"""GPU: the contribution statistics in HIP (csrc/contrib.hip; mojosplat_amd/contrib.py, backend="hip") against the float64
definition on the same HIP-made lists.  The bars, the near-threshold marks and the cases: tests/contrib_cases.py."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import mojosplat_amd as ms
from contrib_cases import (EXCUSED_CAP, Reference, case_camera, case_scene, float32_definition, two_clusters, weight_map,
                           worst_error)
from helpers import assert_grad_close, simple_camera
from mojosplat_amd import (ContributionStats, accumulate_contributions, contributions_from_lists, lift_mask, load_ply, save_ply)
from mojosplat_amd.autograd import render_gaussians_trainable
from mojosplat_amd.binning import bin_gaussians_to_tiles_hip
from mojosplat_amd.projection import project_gaussians_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUFFERS = ("pixels", "max_weight", "sum_q", "wsum_q")


@functools.lru_cache(maxsize=None)
def _hip_lists(case, shift=0.0):
    """The case's lists from the HIP stages (camera moved by `shift` along x) -> device lists, their CPU copies, cameras."""
    dev = torch.device("cuda:0")
    (m, s, q, o), (H, W), ts = case_scene(case)
    cam = case_camera(case, device=dev, T=(shift, 0.0, 0.0))
    m, s, q, o = (t.to(dev) for t in (m, s, q, o))
    m2, con, d, r = project_gaussians_hip(m, s, q, o, cam)
    ids, ranges = bin_gaussians_to_tiles_hip(m2, r, d, ts, -(-W // ts), -(-H // ts))
    gpu = (m2, con, o, ranges, ids)
    return gpu, tuple(t.cpu() for t in gpu), cam, case_camera(case, T=(shift, 0.0, 0.0)), ts


@functools.lru_cache(maxsize=None)
def _reference(case, weights):
    """-> (Reference, bar): the float64 definition with its marks, and 8 x the float32 definition's worst error; computed
    once per (case, weight map) on the CPU from the HIP-made lists."""
    _, cpu, _, cam, ts = _hip_lists(case)
    wmap = None if weights is None else weight_map(weights, cam.H, cam.W)
    ref = Reference(*cpu, cam, ts, weights=wmap, float32_sigma_band=case == "G")
    e32 = worst_error(float32_definition(*cpu, cam, ts, weights=wmap), ref, weights is not None)
    return ref, 8.0 * e32


def _hip_stats(case, weights=None, shift=0.0, into=None):
    gpu, _, cam, _, ts = _hip_lists(case, shift)
    st = ContributionStats(gpu[0].shape[0], gpu[0].device) if into is None else into
    wmap = None if weights is None else weight_map(weights, cam.H, cam.W).to(gpu[0].device)
    return contributions_from_lists(st, *gpu, cam, weights=wmap, tile_size=ts, backend="hip")


def _cpu(st):
    return ContributionStats(0, _buffers=tuple(t.cpu() for t in st._all()))


def _compare(case, weights):
    ref, bar = _reference(case, weights)
    got = _cpu(_hip_stats(case, weights))
    N = ref.stats.n
    err = worst_error(got, ref, weights is not None)
    print(f"CONTRIB case={case} weights={weights} N={N} M={_hip_lists(case)[0][4].numel()} near_pairs={ref.near_pairs} "
          f"excused={int(ref.excused.sum())} slack_total={float(ref.slack.sum()):.3g} "
          f"weight_total={float(ref.stats.weight_sum().sum()):.6g} bar={bar:.3g} hip_err={err:.3g}")
    assert int(ref.excused.sum()) <= EXCUSED_CAP * N, "too many near-threshold Gaussians: a condition on the inputs"
    ok = ~ref.excused
    assert torch.equal(got.pixels[ok], ref.stats.pixels[ok])
    assert torch.equal(got.max_weight[ok] == 0, ref.stats.max_weight[ok] == 0)
    assert bar > 0.0
    assert err <= bar, f"case {case}, weights {weights}: HIP error {err:.3g} over the bar {bar:.3g}"
    if weights is None:
        assert not got.wsum_q.any()
    return got, ref


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "F", "G"])
def test_matches_float64_definition(case):
    got, ref = _compare(case, None)
    if case == "C":       # hidden Gaussians come out exactly zero
        never = (ref.stats.pixels == 0) & ~ref.excused
        assert int(never.sum()) > 300
        assert not got.pixels[never].any() and not got.max_weight[never].any() and not got.sum_q[never].any()
    if case == "D":
        assert int(got.pixels[0]) == 80 * 48
    if case == "G":       # every needle crosses the image: blended in well over a hundred pixels, in tiles far from its mean
        con = _hip_lists("G")[1][1].double()
        assert float(((con[:24, 0] * con[:24, 2] - con[:24, 1] ** 2) / (con[:24, 0] * con[:24, 2])).max()) < 1e-3
        assert bool((ref.stats.pixels[:24] > 100).all())


@pytest.mark.parametrize("weights", ["random", "binary", "wild"])
def test_weight_maps(weights):
    got, _ = _compare("B", weights)
    assert got.wsum_q.any() and bool((got.wsum_q <= got.sum_q).all())
    if weights == "wild":
        twin = _cpu(_hip_stats("B", "wild_clamped"))
        for name in BUFFERS:
            assert torch.equal(getattr(got, name), getattr(twin, name)), name


def test_no_entries_leaves_the_buffers_alone():
    gpu, _, cam, _, ts = _hip_lists("E")
    assert gpu[4].numel() == 0
    st = ContributionStats(gpu[0].shape[0], gpu[0].device)
    st.pixels += 3
    st.max_weight += 0.25
    st.sum_q += 12345
    st.wsum_q -= 9
    before = [t.clone() for t in st._all()]
    wmap = weight_map("random", cam.H, cam.W).to(gpu[0].device)
    contributions_from_lists(st, *gpu, cam, weights=wmap, tile_size=ts, backend="hip")
    for a, b in zip(st._all(), before):
        assert torch.equal(a, b)


def test_bitwise_reproducible_and_order_independent():
    a, b = _hip_stats("B", "random"), _hip_stats("B", "random")
    for name in BUFFERS:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    fwd = _hip_stats("A", "random", shift=0.3, into=_hip_stats("A", "random"))
    rev = _hip_stats("A", "random", into=_hip_stats("A", "random", shift=0.3))
    one = _hip_stats("A", "random")
    for name in BUFFERS:
        assert torch.equal(getattr(fwd, name), getattr(rev, name)), name
    assert bool((fwd.pixels >= one.pixels).all()) and bool((fwd.pixels > one.pixels).any())
    assert bool((fwd.max_weight >= one.max_weight).all())


def test_accumulate_is_its_own_stages_then_lists():
    dev = torch.device("cuda:0")
    (m, s, q, o), _, ts = case_scene("B")
    cam = case_camera("B", device=dev)
    m, s, q, o = (t.to(dev) for t in (m, s, q, o))
    wmap = weight_map("random", cam.H, cam.W).to(dev)
    got = accumulate_contributions(ContributionStats(len(o), dev), m, s, q, o, cam, weights=wmap, tile_size=ts, backend="hip")
    want = _hip_stats("B", "random")
    for name in BUFFERS:
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert got.sum_q.any()


def test_cross_check_against_the_colour_gradient():
    """weighted_sum on case A against independent HIP code: channel 0 of dL/dcolours of the differentiable frame under
    L = sum_p weights_p img[p, 0]."""
    dev = torch.device("cuda:0")
    (m, s, q, o), _, ts = case_scene("A")
    cam = case_camera("A", device=dev)
    m, s, q, o = (t.to(dev) for t in (m, s, q, o))
    wmap = weight_map("random", cam.H, cam.W).to(dev)
    st = accumulate_contributions(ContributionStats(len(o), dev), m, s, q, o, cam, weights=wmap, tile_size=ts, backend="hip")
    colours = torch.full((len(o), 3), 0.5, device=dev, requires_grad=True)
    img = render_gaussians_trainable(m, s, q, o, colours, cam, background_color=None, tile_size=ts)
    (wmap * img[..., 0]).sum().backward()
    assert_grad_close("weighted_sum vs dL/dcolour", st.weighted_sum().cpu(), colours.grad[:, 0].double().cpu())


def test_lift_mask_matches_the_definition():
    dev = torch.device("cuda:0")
    m, s, q, o = two_clusters(12)
    mask = torch.zeros(64, 64, dtype=torch.bool)
    mask[:, :32] = True
    want, want_ratio = lift_mask(m, s, q, o, simple_camera(H=64, W=64, f=60.0), mask, backend="torch")
    got, ratio = lift_mask(*(t.to(dev) for t in (m, s, q, o)), simple_camera(device=dev, H=64, W=64, f=60.0), mask.to(dev),
                           backend="hip")
    assert got.is_cuda and torch.equal(got.cpu(), want) and want.tolist() == [True] * 12 + [False] * 12
    assert float((ratio.cpu() - want_ratio).abs().max()) < 1e-4


def test_argument_errors_before_any_launch():
    gpu, cpu, cam, cam_cpu, ts = _hip_lists("A")
    st = ContributionStats(gpu[0].shape[0], gpu[0].device)
    with pytest.raises(ValueError, match="tile_size"):
        contributions_from_lists(st, *gpu, cam, tile_size=64, backend="hip")
    with pytest.raises(ValueError, match="weights is on cpu"):
        contributions_from_lists(st, *gpu, cam, weights=torch.zeros(cam.H, cam.W), backend="hip")
    with pytest.raises(ValueError, match="stats.pixels is on cpu"):
        contributions_from_lists(ContributionStats(st.n), *gpu, cam, backend="hip")
    with pytest.raises(ValueError):
        contributions_from_lists(ContributionStats(st.n), *cpu, cam_cpu, backend="hip")
    assert not st.pixels.any() and not st.sum_q.any()


def test_prune_example(tmp_path):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(9)
    N = 2000
    params = {"means3d": torch.randn(N, 3, generator=g), "scales": torch.full((N, 3), -2.5) + 0.2 * torch.randn(N, 3, generator=g),
              "quats": torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=1),
              "opacities": torch.randn(N, generator=g), "features": torch.rand(N, 1, 3, generator=g)}
    src, dst = str(tmp_path / "scene.ply"), str(tmp_path / "pruned.ply")
    save_ply(src, {k: v.to(dev) for k, v in params.items()})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "prune_ply.py"), src, dst, "--keep-fraction", "0.25",
                          "--min-max-weight", "0.01", "--views", "6", "--width", "160", "--height", "120"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    kept = int(out.stdout.split("kept ")[1].split(" of ")[0])
    assert 0 < kept <= N // 4 and f"of {N} Gaussians" in out.stdout
    pruned = load_ply(dst)
    assert pruned["means3d"].shape == (kept, 3) and pruned["features"].shape == (kept, 1, 3)
