"""GPU: the scene transform in HIP (csrc/transform.hip; mojosplat_amd/edit.py with backend="hip") against its definition
(backend="torch") on the same device and inputs, BIT FOR BIT -- means, scales, quaternions, features, opacities -- at sizes
around the rows of a workgroup, for every K and RGB features and three maps; two calls in a row; untouched inputs; a partial
last workgroup into guard-filled buffers; bases the kernel cannot vectorise on; the special values of tests/test_edit_cpu.py;
view-dependent colour under the transformed camera, and a rendered frame."""
import pytest
import torch

import mojosplat_amd as ms
from mojosplat_amd import _hip, edit
from edit_cases import KEYS, KS, MAPS, SPECIAL_N, same_bits, same_scene, seeded_scene, sizes, special_scene

pytestmark = pytest.mark.gpu

GUARD = 0x5A


@pytest.mark.parametrize("K", KS)
def test_hip_equals_the_definition_bit_for_bit(device, K):
    assert _hip.TRANSFORM_ROWS == 64 and _hip.TRANSFORM_ROWS_K1 == 256          # what edit_cases.sizes() straddles
    for N in sizes(K):
        p = seeded_scene(N, K, device=device)
        before = {k: v.clone() for k, v in p.items()}
        for name, kw in MAPS.items():
            want = ms.transform_scene(p, backend="torch", **kw)
            got = ms.transform_scene(p, **kw)
            again = ms.transform_scene(p, **kw)
            for k in KEYS:
                assert same_bits(got[k], want[k]), f"N={N} K={K} {name}: {k}"
            assert same_scene(again, got), f"N={N} K={K} {name}: two calls differ"
            assert same_scene(p, before), f"N={N} K={K} {name}: an input changed"


def test_outputs_are_new_contiguous_float32_leaves_on_the_device(device):
    for K in (9, None):
        p = seeded_scene(70, K, device=device)
        p["features"].requires_grad_(True)
        out = ms.transform_scene(p, **MAPS["similarity"])
        grad = ms.transform_scene(p, **MAPS["similarity"], requires_grad=True)
        for k in KEYS:
            assert out[k].is_leaf and not out[k].requires_grad and grad[k].is_leaf and grad[k].requires_grad
            assert out[k].is_contiguous() and out[k].dtype == torch.float32 and out[k].device == p[k].device
            assert out[k].shape == p[k].shape and out[k].untyped_storage().data_ptr() != p[k].untyped_storage().data_ptr()


def _guard(shape, device):
    rows = shape[0]
    return torch.full((rows, 4 * (torch.Size(shape).numel() // rows)), GUARD, dtype=torch.uint8, device=device).view(torch.float32).view(shape)


def _untouched(t, n):
    return bool((t[n:].contiguous().view(torch.uint8) == GUARD).all())


@pytest.mark.parametrize("K", (1, 9, 16))
def test_a_partial_last_workgroup_writes_no_row_past_n(device, K):
    """N = 65 (K = 1: 257): the last workgroup holds one row.  Every output gets 100 rows to spare, filled with a guard byte."""
    N, spare = (257 if K == 1 else 65), 100
    p = seeded_scene(N, K, seed=2, device=device)
    kw = MAPS["similarity"]
    want = ms.transform_scene(p, backend="torch", **kw)
    s, R, t = edit._similarity(None, kw["rotation"], kw["translation"], kw["scale"])
    c = edit._Constants(s, R, t, edit._degree_of(K), single=True)
    out = [_guard((N + spare,) + tuple(p[k].shape[1:]), device) for k in ("means3d", "scales", "quats", "features")]
    edit._transform_hip([p[k] for k in KEYS], K, c, out=out)
    for got, k in zip(out, ("means3d", "scales", "quats", "features")):
        assert same_bits(got[:N], want[k]) and _untouched(got, N), k


def _shifted(t):
    """A contiguous copy of ``t`` that starts 4 bytes into an allocation: no 16-byte access can be made on it."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("K", KS)
def test_bases_that_are_not_16_byte_aligned_give_the_same_bits(device, K):
    N = 130
    big = seeded_scene(N + 1, K, seed=3, device=device)
    p = {k: v[1:].clone() for k, v in big.items()}
    want = ms.transform_scene(p, **MAPS["similarity"])
    views = {k: v[1:] for k, v in big.items()}                        # row-offset views: means and scales start 12 bytes in
    assert views["means3d"].data_ptr() % 16 == 12 and all(v.is_contiguous() for v in views.values())
    assert same_scene(ms.transform_scene(views, **MAPS["similarity"]), want)
    shifted = {k: _shifted(v) for k, v in p.items()}                   # every base 4 bytes in, the outputs' too
    assert same_scene(ms.transform_scene(shifted, **MAPS["similarity"]), want)
    kw = MAPS["similarity"]
    c = edit._Constants(*edit._similarity(None, kw["rotation"], kw["translation"], kw["scale"]), edit._degree_of(K), single=True)
    out = [_shifted(torch.zeros_like(p[k])) for k in ("means3d", "scales", "quats", "features")]
    for src in (p, shifted):
        edit._transform_hip([src[k] for k in KEYS], K, c, out=out)
        for got, k in zip(out, ("means3d", "scales", "quats", "features")):
            assert same_bits(got, want[k]), k
            got.zero_()


@pytest.mark.parametrize("K", KS)
def test_special_values_give_the_definitions_bits(device, K):
    p = special_scene(K, device)
    assert p["means3d"].shape[0] == SPECIAL_N
    for name, kw in MAPS.items():
        want = ms.transform_scene(p, backend="torch", **kw)
        got = ms.transform_scene(p, **kw)
        for k in KEYS:
            assert same_bits(got[k], want[k]), f"K={K} {name}: {k}"
        assert bool(torch.isnan(got["means3d"][0]).any()) and bool(torch.isfinite(got["quats"][3:]).all())


def _camera(device):
    eye = torch.tensor([2.4, -1.8, 5.2])
    vm = ms.look_at(eye, torch.zeros(3), torch.tensor([0.0, 1.0, 0.0])).to(device)
    return ms.Camera(R=vm[:3, :3].contiguous(), T=vm[:3, 3].contiguous(), H=64, W=64, fx=70.0, fy=70.0, cx=32.0, cy=32.0)


def test_colour_is_invariant_under_the_transformed_camera_on_the_device(device):
    """16 products with |b_k| < 3 and a few float32 roundings each on both sides: about 2.3e-5 max |c|; the bound has a 4x
    margin.  The scene stays at least 0.5 away from the camera centre, so that the direction's normalisation is well
    conditioned."""
    p = seeded_scene(2000, 16, seed=4, device=device)
    p["means3d"] = 0.5 * p["means3d"]
    cam = _camera(device)
    centre = torch.tensor(cam._campos(), device=device)
    assert float((p["means3d"] - centre).norm(dim=1).min()) >= 0.5
    want = ms.evaluate_sh(p["means3d"], p["features"], cam, 3, clamp=False, backend="hip")
    scale = float(p["features"].abs().max())
    for name, kw in MAPS.items():
        q = ms.transform_scene(p, **kw)
        got = ms.evaluate_sh(q["means3d"], q["features"], ms.transform_camera(cam, **kw), 3, clamp=False, backend="hip")
        err = float((got - want).abs().max())
        print(f"{name}: colour error {err / scale:.2e} max |c|")
        assert err <= 1e-4 * scale
    stale = ms.evaluate_sh(q["means3d"], p["features"], ms.transform_camera(cam, **kw), 3, clamp=False, backend="hip")
    assert float((stale - want).abs().max()) > 1e-2 * scale          # the coefficients left alone: wrong colour


def test_a_frame_of_the_transformed_scene_is_the_same_for_both_backends(device):
    p = seeded_scene(500, 16, seed=5, device=device)
    p["means3d"] = 0.4 * p["means3d"]
    p["scales"] = p["scales"] - 1.5
    p["features"][:, 1:] *= 0.2
    kw = MAPS["similarity"]
    cam = ms.transform_camera(_camera(device), **kw)
    frames = []
    with torch.no_grad():
        for backend in ("hip", "torch"):
            q = ms.transform_scene(p, backend=backend, **kw)
            frames.append(ms.render_gaussians(q["means3d"], q["scales"], q["quats"], torch.sigmoid(q["opacities"]), q["features"], cam,
                                              sh_degree=3, backend="hip"))
    assert frames[0].shape[:2] == (64, 64) and same_bits(frames[0], frames[1])
    assert float(frames[0].max()) > 0.05                             # ... and something was drawn
